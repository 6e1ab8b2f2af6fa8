// vaa_jpeg.hip — K12: the JPEG round trip of camera frames [B,H,W,3] uint8 in front of K8 (include/vaa.h states the arithmetic, step by
// step; this file follows its numbering). Only the lossy chain of a baseline 4:2:0 codec is computed — colour conversion, subsampling, forward
// DCT, quantise / dequantise, inverse DCT, "fancy" upsampling, colour conversion back — in int32 throughout; no entropy coder, no file.
//
// Replaces, per camera frame of the reference's LIBERO evaluation, tf.io.encode_jpeg + tf.io.decode_image in resize_image
// (experiments/robot/libero/libero_utils.py:42-43) and, with rot180, the img[::-1, ::-1] in front of it.
//
// Shape: a 256-thread workgroup owns 32 8x8 blocks, one (block, row) or (block, column) per lane. The blocks live in LDS as int32 with a row
// pitch of 9 dwords: the eight rows (or columns) that the lanes of a block read, and the eight blocks of a wave (72*b = 8*b mod 64), then fall
// into 64 different banks. A lane runs the eight-point pass of its row in registers, the transpose is the LDS itself, and the column pass
// runs forward DCT, quantise, dequantise and the inverse column pass on one register set: a coefficient never leaves the registers.
//   launch 1  jpeg_chroma_kernel: 16 MCUs of one MCU row per workgroup (16 Cb + 16 Cr blocks). Every thread subsamples 4 chroma positions from
//             their 2x2 pixels; the decoded half-resolution planes go to the workspace (8 bytes per lane, one store).
//   launch 2  jpeg_luma_finish_kernel: 8 MCUs of one MCU row per workgroup (32 Y blocks). The decoded Y tile stays in LDS; the chroma samples
//             of the tile plus one sample on every side come from the workspace (clamped to the FRAME's half-resolution size: the upsampling's
//             edges are the frame's), then per 4 pixels: triangle filter, colour conversion, three dword stores (bytes when W % 4 != 0).
// The decoder's upsampling reads one decoded chroma sample beyond each block edge, which is why there are two launches and a workspace
// (profiles/EXPERIMENTS.md: the alternative is a workgroup that decodes its neighbours' chroma blocks again).
// No atomics, no hand-over between workgroups inside a launch, no inline assembly, no floating point.
#include "vaa_common.h"

namespace vaa {

constexpr int kJpThreads = 256;
constexpr int kJpBlocks = 32;                 // 8x8 blocks per workgroup
constexpr int kJpPitch = 9;                   // dwords per block row
constexpr int kJpBlockDw = 8 * kJpPitch;      // 72
constexpr int kJpChromaMcus = 16;             // MCUs per workgroup, launch 1
constexpr int kJpLumaMcus = 8;                // MCUs per workgroup, launch 2
constexpr int kJpTileW = kJpLumaMcus * 16;    // 128 pixels
constexpr int kJpCsW = kJpTileW / 2 + 2;      // 66 staged chroma columns
constexpr int kJpCsH = 10;                    // 8 + 2 staged chroma rows
constexpr int kJpMinSide = 8, kJpMaxSide = 2048;

constexpr int kC298 = 2446, kC390 = 3196, kC541 = 4433, kC765 = 6270, kC899 = 7373, kC1175 = 9633;
constexpr int kC1501 = 12299, kC1847 = 15137, kC1961 = 16069, kC2053 = 16819, kC2562 = 20995, kC3072 = 25172;

struct JpegArgs {
    const uint8_t* src;
    uint8_t* dst;
    const uint16_t* qtab;  // [2][64]
    uint8_t* ws;           // [B][2][8*MY][8*MX]
    int H, W, MX, MY, rot, tiles;  // tiles: workgroups per MCU row
};

__device__ __forceinline__ int jp_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// step 3: one eight-point forward pass
template <bool kRows>
__device__ __forceinline__ void jp_fdct8(int (&d)[8]) {
    constexpr int n = kRows ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kRows) {
        d[0] = (t10 + t11) << 2;
        d[4] = (t10 - t11) << 2;
    } else {
        d[0] = jp_descale(t10 + t11, 2);
        d[4] = jp_descale(t10 - t11, 2);
    }
    const int ze = (t12 + t13) * kC541;
    d[2] = jp_descale(ze + t13 * kC765, n);
    d[6] = jp_descale(ze - t12 * kC1847, n);
    const int z5 = ((t4 + t6) + (t5 + t7)) * kC1175;
    const int z1 = (t4 + t7) * -kC899, z2 = (t5 + t6) * -kC2562;
    const int z3 = (t4 + t6) * -kC1961 + z5, z4 = (t5 + t7) * -kC390 + z5;
    d[7] = jp_descale(t4 * kC298 + z1 + z3, n);
    d[5] = jp_descale(t5 * kC2053 + z2 + z4, n);
    d[3] = jp_descale(t6 * kC3072 + z2 + z3, n);
    d[1] = jp_descale(t7 * kC1501 + z1 + z4, n);
}

// step 5: one eight-point inverse pass
template <bool kCols>
__device__ __forceinline__ void jp_idct8(int (&d)[8]) {
    constexpr int n = kCols ? 11 : 18;
    const int ze = (d[2] + d[6]) * kC541;
    const int t2 = ze - d[6] * kC1847, t3 = ze + d[2] * kC765;
    const int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int u0 = d[7], u1 = d[5], u2 = d[3], u3 = d[1];
    const int z5 = ((u0 + u2) + (u1 + u3)) * kC1175;
    const int z1 = (u0 + u3) * -kC899, z2 = (u1 + u2) * -kC2562;
    const int z3 = (u0 + u2) * -kC1961 + z5, z4 = (u1 + u3) * -kC390 + z5;
    u0 = u0 * kC298 + z1 + z3;
    u1 = u1 * kC2053 + z2 + z4;
    u2 = u2 * kC3072 + z2 + z3;
    u3 = u3 * kC1501 + z1 + z4;
    d[0] = jp_descale(t10 + u3, n); d[7] = jp_descale(t10 - u3, n);
    d[1] = jp_descale(t11 + u2, n); d[6] = jp_descale(t11 - u2, n);
    d[2] = jp_descale(t12 + u1, n); d[5] = jp_descale(t12 - u1, n);
    d[3] = jp_descale(t13 + u0, n); d[4] = jp_descale(t13 - u0, n);
}

// Steps 3-5 for the workgroup's 32 blocks (blk: [32][8][9] level-shifted samples; qt: the component's 64 table entries in LDS). Lane (b, l)
// returns the decoded samples 0..255 of row l of block b. The caller places a barrier between its fill of blk and this call.
__device__ __forceinline__ void jp_block_roundtrip(int* blk, const int* qt, int tid, int (&d)[8]) {
    const int l = tid & 7;
    int* p = blk + (tid >> 3) * kJpBlockDw;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[l * kJpPitch + j];
    jp_fdct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[l * kJpPitch + j] = d[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i * kJpPitch + l];
    jp_fdct8<false>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // step 4
        const unsigned q = (unsigned)qt[i * 8 + l];
        const unsigned mag = (unsigned)(d[i] < 0 ? -d[i] : d[i]);
        const int v = (int)(((mag + 4u * q) / (8u * q)) * q);
        d[i] = d[i] < 0 ? -v : v;
    }
    jp_idct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i * kJpPitch + l] = d[i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[l * kJpPitch + j];
    jp_idct8<false>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = min(max(d[j] + 128, 0), 255);
}

// pixel (y, x) of the frame that is encoded, y < H, x < W: R | G << 8 | B << 16
__device__ __forceinline__ uint32_t jp_pixel(const JpegArgs& a, int b, int y, int x) {
    const int sy = a.rot ? a.H - 1 - y : y, sx = a.rot ? a.W - 1 - x : x;
    const uint8_t* p = a.src + (((size_t)b * a.H + sy) * a.W + sx) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ __forceinline__ void jp_load_qtab(const JpegArgs& a, int* qs, int tid) {
    if (tid < 128) qs[tid] = max((int)a.qtab[tid], 1);
}

__global__ __launch_bounds__(kJpThreads) void jpeg_chroma_kernel(const JpegArgs a) {
    __shared__ int blk[kJpBlocks * kJpBlockDw];
    __shared__ int qs[128];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles, my = (blockIdx.x / a.tiles) % a.MY, b = blockIdx.x / (a.tiles * a.MY);
    const int H = a.H, W = a.W, ch = (H + 1) >> 1;
    jp_load_qtab(a, qs, tid);
    // steps 1, 2: 8 x 128 subsampled positions, four per thread, Cb and Cr of each
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = tid + k * kJpThreads, i = s >> 7, jj = s & 127;
        const int j = tx * (kJpChromaMcus * 8) + jj, ic = min(my * 8 + i, ch - 1);
        const int y0 = min(2 * ic, H - 1), y1 = min(2 * ic + 1, H - 1), x0 = min(2 * j, W - 1), x1 = min(2 * j + 1, W - 1);
        int cb = 0, cr = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t px = jp_pixel(a, b, (e & 2) ? y1 : y0, (e & 1) ? x1 : x0);
            const int R = px & 255, G = (px >> 8) & 255, B = (px >> 16) & 255;
            cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
        const int bias = 1 + (j & 1);
        int* p = blk + ((jj >> 3) * 2) * kJpBlockDw + i * kJpPitch + (jj & 7);
        p[0] = ((cb + bias) >> 2) - 128;
        p[kJpBlockDw] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    int d[8];
    jp_block_roundtrip(blk, qs + 64, tid, d);
    const int bi = tid >> 3, m = tx * kJpChromaMcus + (bi >> 1);
    if (m < a.MX) {
        const size_t CW = (size_t)a.MX * 8, CH = (size_t)a.MY * 8;
        uint2 v;
        v.x = (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        v.y = (uint32_t)d[4] | ((uint32_t)d[5] << 8) | ((uint32_t)d[6] << 16) | ((uint32_t)d[7] << 24);
        *reinterpret_cast<uint2*>(a.ws + (((size_t)b * 2 + (bi & 1)) * CH + my * 8 + (tid & 7)) * CW + (size_t)m * 8) = v;
    }
}

__global__ __launch_bounds__(kJpThreads) void jpeg_luma_finish_kernel(const JpegArgs a) {
    __shared__ int blk[kJpBlocks * kJpBlockDw];
    __shared__ int qs[128];
    __shared__ uint32_t ydec[16 * (kJpTileW / 4)];      // the decoded Y tile, 16 rows of 128 bytes
    __shared__ uint8_t cs[2 * kJpCsH * kJpCsW];         // decoded chroma of the tile with one sample on every side
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles, my = (blockIdx.x / a.tiles) % a.MY, b = blockIdx.x / (a.tiles * a.MY);
    const int H = a.H, W = a.W, ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    jp_load_qtab(a, qs, tid);
    // step 1: the tile's 16 x 128 Y samples, eight per thread
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = tid + k * kJpThreads, r = s >> 7, xx = s & 127;
        const uint32_t px = jp_pixel(a, b, min(my * 16 + r, H - 1), min(tx * kJpTileW + xx, W - 1));
        const int R = px & 255, G = (px >> 8) & 255, B = (px >> 16) & 255;
        const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        blk[((xx >> 4) * 4 + (r >> 3) * 2 + ((xx >> 3) & 1)) * kJpBlockDw + (r & 7) * kJpPitch + (xx & 7)] = Y - 128;
    }
    {
        const size_t CW = (size_t)a.MX * 8, CH = (size_t)a.MY * 8;
        for (int e = tid; e < 2 * kJpCsH * kJpCsW; e += kJpThreads) {
            const int c = e / (kJpCsH * kJpCsW), rem = e - c * (kJpCsH * kJpCsW), i = rem / kJpCsW, j = rem - i * kJpCsW;
            const int gi = min(max(my * 8 - 1 + i, 0), ch - 1), gj = min(max(tx * (kJpTileW / 2) - 1 + j, 0), cw - 1);
            cs[e] = a.ws[(((size_t)b * 2 + c) * CH + gi) * CW + gj];
        }
    }
    __syncthreads();
    int d[8];
    jp_block_roundtrip(blk, qs, tid, d);
    {
        const int bi = tid >> 3, row = ((bi >> 1) & 1) * 8 + (tid & 7), col4 = (bi >> 2) * 4 + (bi & 1) * 2;
        ydec[row * (kJpTileW / 4) + col4] = (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        ydec[row * (kJpTileW / 4) + col4 + 1] = (uint32_t)d[4] | ((uint32_t)d[5] << 8) | ((uint32_t)d[6] << 16) | ((uint32_t)d[7] << 24);
    }
    __syncthreads();
    // steps 6, 7: groups of four pixels, two per thread
    const bool wide = (W & 3) == 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int g = tid + k * kJpThreads, r = g >> 5, xq = (g & 31) * 4;
        const int gy = my * 16 + r, gx = tx * kJpTileW + xq;
        if (gy >= H || gx >= W) continue;
        const uint32_t y4 = ydec[r * (kJpTileW / 4) + (xq >> 2)];
        const int i1 = (r >> 1) + 1, i2 = (r & 1) ? i1 + 1 : i1 - 1;  // staged rows: the sample's own and its vertical neighbour
        uint8_t o[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int x = xq + p, j1 = (x >> 1) + 1, j2 = (x & 1) ? j1 + 1 : j1 - 1, rnd = (x & 1) ? 7 : 8;
            int cc[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* t = cs + c * (kJpCsH * kJpCsW);
                const int s1 = 3 * t[i1 * kJpCsW + j1] + t[i2 * kJpCsW + j1], s2 = 3 * t[i1 * kJpCsW + j2] + t[i2 * kJpCsW + j2];
                cc[c] = ((3 * s1 + s2 + rnd) >> 4) - 128;
            }
            const int Y = (y4 >> (8 * p)) & 255;
            o[3 * p + 0] = (uint8_t)min(max(Y + ((91881 * cc[1] + 32768) >> 16), 0), 255);
            o[3 * p + 1] = (uint8_t)min(max(Y + ((-22554 * cc[0] + 32768 - 46802 * cc[1]) >> 16), 0), 255);
            o[3 * p + 2] = (uint8_t)min(max(Y + ((116130 * cc[0] + 32768) >> 16), 0), 255);
        }
        uint8_t* q = a.dst + (((size_t)b * H + gy) * W + gx) * 3;
        if (wide) {  // W % 4 == 0: gx + 3 < W and the 12 bytes start on a dword
            uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
#pragma unroll
            for (int z = 0; z < 3; ++z)
                q4[z] = (uint32_t)o[4 * z] | ((uint32_t)o[4 * z + 1] << 8) | ((uint32_t)o[4 * z + 2] << 16) | ((uint32_t)o[4 * z + 3] << 24);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (gx + p < W) {
                    q[3 * p] = o[3 * p]; q[3 * p + 1] = o[3 * p + 1]; q[3 * p + 2] = o[3 * p + 2];
                }
        }
    }
}

static bool jpeg_sizes_ok(int B, int H, int W) {
    if (B < 0 || H < kJpMinSide || H > kJpMaxSide || W < kJpMinSide || W > kJpMaxSide) return false;
    const long MX = (W + 15) / 16, MY = (H + 15) / 16;
    return (long)B * MY * ((MX + kJpLumaMcus - 1) / kJpLumaMcus) <= 0x7fffffffL;
}

}  // namespace vaa

extern "C" size_t vaa_jpeg_roundtrip_ws_bytes(int B, int H, int W) {
    if (!vaa::jpeg_sizes_ok(B, H, W)) return 0;
    return (size_t)B * 2 * (size_t)(8 * ((H + 15) / 16)) * (size_t)(8 * ((W + 15) / 16));
}

extern "C" int vaa_jpeg_roundtrip(const uint8_t* src_u8, int B, int H, int W, int rot180, const uint16_t* qtab_host, const uint16_t* qtab_dev,
                                  uint8_t* dst_u8, void* ws, size_t ws_bytes, void* stream) {
    using namespace vaa;
    const char* who = "vaa_jpeg_roundtrip";
    if (B < 0) {
        set_error("%s: bad batch size (B=%d)", who, B);
        return VAA_E_INVALID;
    }
    if (B == 0) return VAA_OK;  // empty batch: nothing to read or write (pointers may be null)
    if (!jpeg_sizes_ok(B, H, W)) {
        set_error("%s: frames of %dx%d outside [%d, %d] per side, or B=%d beyond the grid", who, H, W, kJpMinSide, kJpMaxSide, B);
        return VAA_E_INVALID;
    }
    if (rot180 != 0 && rot180 != 1) {
        set_error("%s: rot180 must be 0 or 1 (got %d)", who, rot180);
        return VAA_E_INVALID;
    }
    if (!src_u8 || !qtab_host || !qtab_dev || !dst_u8) {
        set_error("%s: null pointer argument", who);
        return VAA_E_INVALID;
    }
    if (((uintptr_t)src_u8 & 3u) || ((uintptr_t)dst_u8 & 3u) || ((uintptr_t)qtab_dev & 1u)) {
        set_error("%s: src_u8 and dst_u8 must be 4-byte and qtab_dev 2-byte aligned", who);
        return VAA_E_INVALID;
    }
    {   // a workgroup of launch 2 writes dst while others still read src: no byte of src may lie inside dst (K11's rule, by address ranges)
        const size_t nb = (size_t)B * H * W * 3;
        const uintptr_t i0 = (uintptr_t)src_u8, o0 = (uintptr_t)dst_u8;
        if (i0 < o0 + nb && o0 < i0 + nb) {
            set_error("%s: src_u8 and dst_u8 must not overlap", who);
            return VAA_E_INVALID;
        }
    }
    for (int i = 0; i < 128; ++i)
        if (qtab_host[i] < 1 || qtab_host[i] > 255) {
            set_error("%s: quantisation table %d entry %d is %d, outside 1..255", who, i >> 6, i & 63, (int)qtab_host[i]);
            return VAA_E_INVALID;
        }
    const size_t need = vaa_jpeg_roundtrip_ws_bytes(B, H, W);
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < need) {
        set_error("%s: workspace missing, not 8-byte aligned or too small (%zu < %zu bytes)", who, ws ? ws_bytes : (size_t)0, need);
        return VAA_E_WORKSPACE;
    }

    JpegArgs a = {};
    a.src = src_u8; a.dst = dst_u8; a.qtab = qtab_dev; a.ws = static_cast<uint8_t*>(ws);
    a.H = H; a.W = W; a.MX = (W + 15) / 16; a.MY = (H + 15) / 16; a.rot = rot180;
    a.tiles = (a.MX + kJpChromaMcus - 1) / kJpChromaMcus;
    VAA_LAUNCH(jpeg_chroma_kernel, dim3((unsigned)(B * a.MY * a.tiles)), dim3(kJpThreads), 0, (hipStream_t)stream, a);
    int rc = check_launch(who);
    if (rc != VAA_OK) return rc;
    a.tiles = (a.MX + kJpLumaMcus - 1) / kJpLumaMcus;
    VAA_LAUNCH(jpeg_luma_finish_kernel, dim3((unsigned)(B * a.MY * a.tiles)), dim3(kJpThreads), 0, (hipStream_t)stream, a);
    return check_launch(who);
}
