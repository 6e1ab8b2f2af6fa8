// vaa_quant8.hip — the 8-bit Llama projections of the evaluation path (include/vaa_model_ops.h: vaa_model_q8_act_quant, vaa_model_q8_matmul):
// int8 weights with one fp32 scale per row, activations quantised per row on every call, integer products on the matrix cores
// (mfma_i32_16x16x64_i8), the columns whose activations reach the threshold carried in bf16. Inference only. The header states the format and
// every arithmetic step; this file is built with -ffp-contract=off and correctly rounded division, so each step is one IEEE operation.
//
// vaa_model_q8_act_quant. A thread owns 16 bytes of a row (8 columns); a workgroup owns one row m.
//   M <= 16 (a decode step), ONE launch: every workgroup forms the column maxima of all M rows itself (x is M * K * 2 <= 352 KB, L2 resident),
//     keeps the outlier columns as a bitmap in LDS, takes its row's maximum over the other columns, and quantises its row; workgroup 0 also
//     writes the ordered list from the bitmap (a block scan per 8192 columns: the order is fixed).
//   M > 16 (prefill), three launches: q8_colflag_kernel (16 column vectors x 16 row lanes per workgroup) writes one 0/1 word per column into
//     the caller's K + 1 words; the row kernel reads them into its bitmap; q8_compact_kernel (one workgroup) reads ALL of them into its bitmap,
//     then overwrites the words with the count and the ordered list.
//   Maxima do not depend on order and the list is built by a scan, so nothing here depends on timing.
//
// vaa_model_q8_matmul, A = q (rows n), B = xq^T (columns m), C[row n][col m] int32. Both operands are K-contiguous: lane (r = lane & 15,
// g = lane >> 4) loads the 16 bytes at k0 + 16 g of row n0 + r of q and of row m0 + r of xq straight into the fragments of one MFMA. The slot
// (g, byte) of A and of B holds the same k, and an integer sum does not depend on the order of its terms.
//   M <= 16: q8_gemv_kernel, the layout of q4_gemv_kernel. A workgroup of 8 waves owns 16 rows n; the K axis is cut into tiles of 128 elements
//     (two MFMAs) and tile t belongs to wave t % 8, so one round of the workgroup is 1024 elements; two tiles' loads are in flight. Every weight
//     byte is read once, by one lane of one workgroup. The 8 int32 partial tiles meet in LDS; one thread per output sums them and runs the
//     epilogue.
//   M > 16: q8_gemm_kernel. A workgroup of 4 waves owns 128 rows n x 64 rows m, a wave 32 x 64 (2 x 4 accumulator tiles): six 16-byte loads
//     feed eight MFMAs per 64 elements of K, operands straight from L2 (the four waves share the xq tile through the cache). The weights are
//     read ceil(M / 64) times. No LDS, no barrier.
//   Rows m >= M, rows n >= N and the K slots past K of a ragged last tile are zeros that no load touches. Both kernels end in the same device
//   functions (q8_wdq, q8_finish; the GEMM advances a thread's 32 outlier sums together, each in q8_epilogue's order): the scales, the outlier
//   sum in ascending column order, res, one rounding — the same bits from either form. The outlier sum costs one gather per outlier column
//   and output (GEMM: per 8 x 4 outputs); it is meant for the few columns a threshold of 6 leaves.
#include <cmath>

#include "vaa_common.h"
#include "../../include/vaa_model_ops.h"

namespace vaa {

typedef int q8_v4i __attribute__((ext_vector_type(4)));

constexpr int kQ8MaxK = 133120;  // 127^2 * K < 2^31
constexpr int kQ8ActThreads = 256, kQ8SmallM = 16;
constexpr int kQ8FlagCols = 16, kQ8FlagRows = 16;  // q8_colflag_kernel: column vectors x row lanes per workgroup
constexpr int kQ8GemvWaves = 8, kQ8GemvThreads = 64 * kQ8GemvWaves, kQ8GemvRows = 16, kQ8GemvTileK = 128;
constexpr int kQ8GemmThreads = 256, kQ8GemmN = 128, kQ8GemmM = 64;

// 16 bytes = 8 consecutive bf16 (element 2i in the low half of dword i) -> fp32
__device__ __forceinline__ void q8_unpack8(const uint4& d, float* f) {
    const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bf16_bits_to_f32((dw[e >> 1] >> (16 * (e & 1))) & 0xffffu);
}

// xq = clamp(rint(x * inv), -127, 127): one product, one rounding to an integer
__device__ __forceinline__ int q8_quant1(float x, float inv) {
    const float v = rintf(x * inv);
    return (int)fminf(fmaxf(v, -127.0f), 127.0f);
}

// The ordered list from the bitmap (bit e of byte v = column 8 v + e), by all kQ8ActThreads threads of ONE workgroup: a thread owns 32
// consecutive columns of a chunk of 8192, the chunk's counts are scanned in LDS, every thread writes its columns in ascending order.
__device__ __forceinline__ void q8_compact(const uint8_t* s_bits, int nv, int32_t* __restrict__ outliers, int* s_scan) {
    const int tid = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < nv; b0 += 4 * kQ8ActThreads) {
        const int b = b0 + 4 * tid;
        uint32_t mask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (b + j < nv) mask |= (uint32_t)s_bits[b + j] << (8 * j);
        const int c = __popc(mask);
        s_scan[tid] = c;
        __syncthreads();
        for (int off = 1; off < kQ8ActThreads; off <<= 1) {
            const int add = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        int pos = base + s_scan[tid] - c;
        base += s_scan[kQ8ActThreads - 1];
        while (mask) {
            const int bit = __ffs((int)mask) - 1;
            mask &= mask - 1;
            outliers[1 + pos++] = 8 * b + bit;  // pos < count <= K: inside the K + 1 words
        }
        __syncthreads();
    }
    if (tid == 0) outliers[0] = base;
}

// One 0/1 word per column: outliers[1 + k] = (t > 0 and max_m |x[m, k]| >= t).
__global__ __launch_bounds__(kQ8FlagCols* kQ8FlagRows) void q8_colflag_kernel(const uint16_t* __restrict__ x, int M, int K, float t,
                                                                             int32_t* __restrict__ outliers) {
    __shared__ float s_c[kQ8FlagRows][kQ8FlagCols][8];
    const int cv = threadIdx.x % kQ8FlagCols, rl = threadIdx.x / kQ8FlagCols;
    const int nv = K / 8, v = blockIdx.x * kQ8FlagCols + cv;
    float cmax[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (v < nv && t > 0.0f) {
        for (int mm = rl; mm < M; mm += kQ8FlagRows) {
            float f[8];
            q8_unpack8(*reinterpret_cast<const uint4*>(x + (long)mm * K + 8 * v), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) cmax[e] = fmaxf(cmax[e], fabsf(f[e]));
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_c[rl][cv][e] = cmax[e];
    __syncthreads();
    if (rl == 0 && v < nv) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float c = 0.0f;
            for (int i = 0; i < kQ8FlagRows; ++i) c = fmaxf(c, s_c[i][cv][e]);
            outliers[1 + 8 * v + e] = (t > 0.0f && c >= t) ? 1 : 0;
        }
    }
}

// Row m = blockIdx.x: the outlier bitmap (kFlags: from the words q8_colflag_kernel wrote; else from the column maxima of all M <= 16 rows),
// ascale[m], xq[m, :]. Without kFlags, workgroup 0 also writes the ordered list.
template <bool kFlags>
__global__ __launch_bounds__(kQ8ActThreads) void q8_rows_kernel(const uint16_t* __restrict__ x, int M, int K, float t, int8_t* __restrict__ xq,
                                                                float* __restrict__ ascale, int32_t* __restrict__ outliers) {
    __shared__ uint8_t s_bits[kQ8MaxK / 8];
    __shared__ float s_max[kQ8ActThreads / 64];
    __shared__ int s_scan[kQ8ActThreads];
    const int tid = threadIdx.x, m = blockIdx.x, nv = K / 8;
    const uint16_t* xr = x + (long)m * K;
    float rmax = 0.0f;
    for (int v = tid; v < nv; v += kQ8ActThreads) {
        uint32_t bits = 0;
        float f[8];
        if (kFlags) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bits |= (outliers[1 + 8 * v + e] != 0 ? 1u : 0u) << e;
        } else if (t > 0.0f) {
            float cmax[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int mm = 0; mm < M; ++mm) {
                q8_unpack8(*reinterpret_cast<const uint4*>(x + (long)mm * K + 8 * v), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) cmax[e] = fmaxf(cmax[e], fabsf(f[e]));
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) bits |= (cmax[e] >= t ? 1u : 0u) << e;
        }
        s_bits[v] = (uint8_t)bits;
        q8_unpack8(*reinterpret_cast<const uint4*>(xr + 8 * v), f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (!((bits >> e) & 1u)) rmax = fmaxf(rmax, fabsf(f[e]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, off));
    if ((tid & 63) == 0) s_max[tid >> 6] = rmax;
    __syncthreads();
    float as = s_max[0];
#pragma unroll
    for (int i = 1; i < kQ8ActThreads / 64; ++i) as = fmaxf(as, s_max[i]);
    if (tid == 0) ascale[m] = as;
    const float inv = as > 0.0f ? 127.0f / as : 0.0f;  // the one division of the row
    for (int v = tid; v < nv; v += kQ8ActThreads) {
        const uint32_t bits = s_bits[v];
        float f[8];
        q8_unpack8(*reinterpret_cast<const uint4*>(xr + 8 * v), f);
        uint32_t o[2] = {0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int qv = (((bits >> e) & 1u) || !(as > 0.0f)) ? 0 : q8_quant1(f[e], inv);
            o[e >> 2] |= ((uint32_t)qv & 0xffu) << (8 * (e & 3));
        }
        *reinterpret_cast<uint2*>(xq + (long)m * K + 8 * v) = make_uint2(o[0], o[1]);
    }
    if (!kFlags && m == 0) q8_compact(s_bits, nv, outliers, s_scan);  // s_bits is complete: the barrier above
}

// One workgroup: all K flag words into the bitmap, THEN the count and the ordered list over the same words.
__global__ __launch_bounds__(kQ8ActThreads) void q8_compact_kernel(int K, int32_t* __restrict__ outliers) {
    __shared__ uint8_t s_bits[kQ8MaxK / 8];
    __shared__ int s_scan[kQ8ActThreads];
    const int nv = K / 8;
    for (int v = threadIdx.x; v < nv; v += kQ8ActThreads) {
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) bits |= (outliers[1 + 8 * v + e] != 0 ? 1u : 0u) << e;
        s_bits[v] = (uint8_t)bits;
    }
    __syncthreads();
    q8_compact(s_bits, nv, outliers, s_scan);
}

// The epilogue of both matmul forms, in three device functions that each form calls with the same scalars (the header states every step):
// the outlier count, one dequantised weight, and y[m, n] from the exact integer sum and the finished outlier sum.
__device__ __forceinline__ int q8_outlier_count(const int32_t* __restrict__ outliers, int K) {
    return min(outliers[0], K);  // a list that vaa_model_q8_act_quant did not write cannot lead outside x, q or the K + 1 words
}

__device__ __forceinline__ int q8_outlier_col(const int32_t* __restrict__ outliers, int j, int K) { return min(max(outliers[1 + j], 0), K - 1); }

__device__ __forceinline__ float q8_wdq(int8_t qv, float ws) { return bf16_bits_to_f32(f32_to_bf16_bits(((float)qv * ws) / 127.0f)); }

__device__ __forceinline__ uint16_t q8_finish(int acc, float as, float ws, float o, const uint16_t* __restrict__ res, long at) {
    float yv = ((float)acc * (as * ws)) / 16129.0f + o;
    if (res) yv = yv + bf16_bits_to_f32(res[at]);
    return (uint16_t)f32_to_bf16_bits(yv);
}

// One output: the outlier sum in ascending column order, then q8_finish.
__device__ __forceinline__ uint16_t q8_epilogue(int acc, int m, int n, int N, int K, const float* __restrict__ ascale, const float* __restrict__ wscale,
                                                const int32_t* __restrict__ outliers, const uint16_t* __restrict__ x, const int8_t* __restrict__ q,
                                                const uint16_t* __restrict__ res) {
    const float ws = wscale[n];
    const int cnt = q8_outlier_count(outliers, K);
    float o = 0.0f;
    for (int j = 0; j < cnt; ++j) {
        const int k = q8_outlier_col(outliers, j, K);
        o = o + bf16_bits_to_f32(x[(long)m * K + k]) * q8_wdq(q[(long)n * K + k], ws);
    }
    return q8_finish(acc, ascale[m], ws, o, res, (long)m * N + n);
}

struct Q8Tile {
    uint4 a[2];  // q[n0 + r][k0 + 64 j + 16 g .. + 15]
    uint4 b[2];  // xq[r][the same 16 elements]
};

// Tile t of the K axis for lane (r, g): zeros (and no load) past the last tile, past K in a ragged last tile, for rows n >= N and m >= M.
__device__ __forceinline__ void q8_load_tile(Q8Tile& q, int t, int tiles, int K, int g, bool wrow, bool xrow, const int8_t* __restrict__ qrow,
                                             const int8_t* __restrict__ xrow_p) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k0 = t * kQ8GemvTileK + 64 * j + 16 * g;
        const bool live = t < tiles && k0 < K;  // K % 64 == 0 and k0 % 16 == 0: k0 < K means k0 + 16 <= K
        q.a[j] = make_uint4(0u, 0u, 0u, 0u);
        q.b[j] = make_uint4(0u, 0u, 0u, 0u);
        if (live && wrow) q.a[j] = *reinterpret_cast<const uint4*>(qrow + k0);
        if (live && xrow) q.b[j] = *reinterpret_cast<const uint4*>(xrow_p + k0);
    }
}

__device__ __forceinline__ q8_v4i q8_tile_mfma(const Q8Tile& q, q8_v4i acc) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const q8_v4i*>(&q.a[j]), *reinterpret_cast<const q8_v4i*>(&q.b[j]), acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(kQ8GemvThreads) void q8_gemv_kernel(const int8_t* __restrict__ xq, const float* __restrict__ ascale,
                                                                 const int32_t* __restrict__ outliers, const uint16_t* __restrict__ x, int M,
                                                                 const int8_t* __restrict__ q, const float* __restrict__ wscale, int N, int K,
                                                                 const uint16_t* __restrict__ res, uint16_t* __restrict__ y) {
    __shared__ int s_acc[kQ8GemvWaves][kQ8SmallM][kQ8GemvRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * kQ8GemvRows;
    const bool wrow = n0 + r < N, xrow = r < M;
    const int8_t* qrow = q + (long)(wrow ? n0 + r : 0) * K;
    const int8_t* xr = xq + (long)(xrow ? r : 0) * K;
    const int tiles = (K + kQ8GemvTileK - 1) / kQ8GemvTileK;
    q8_v4i acc = {0, 0, 0, 0};
    for (int t = wave; t < tiles; t += 2 * kQ8GemvWaves) {  // two tiles' loads in flight before the first use
        Q8Tile t0, t1;
        q8_load_tile(t0, t, tiles, K, g, wrow, xrow, qrow, xr);
        q8_load_tile(t1, t + kQ8GemvWaves, tiles, K, g, wrow, xrow, qrow, xr);
        acc = q8_tile_mfma(t0, acc);
        acc = q8_tile_mfma(t1, acc);
    }
    // C layout: col (= m) = lane & 15, row (= n - n0) = 4 * (lane >> 4) + reg
#pragma unroll
    for (int i = 0; i < 4; ++i) s_acc[wave][r][4 * g + i] = acc[i];
    __syncthreads();
    if (tid < kQ8SmallM * kQ8GemvRows) {
        const int m = tid / kQ8GemvRows, n = n0 + tid % kQ8GemvRows;
        if (m < M && n < N) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < kQ8GemvWaves; ++w) s += s_acc[w][m][tid % kQ8GemvRows];  // exact: any order gives the same sum
            y[(long)m * N + n] = q8_epilogue(s, m, n, N, K, ascale, wscale, outliers, x, q, res);
        }
    }
}

__global__ __launch_bounds__(kQ8GemmThreads) void q8_gemm_kernel(const int8_t* __restrict__ xq, const float* __restrict__ ascale,
                                                                 const int32_t* __restrict__ outliers, const uint16_t* __restrict__ x, int M,
                                                                 const int8_t* __restrict__ q, const float* __restrict__ wscale, int N, int K,
                                                                 const uint16_t* __restrict__ res, uint16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * kQ8GemmN + 32 * wave, m0 = blockIdx.y * kQ8GemmM;
    const int8_t* ap[2];
    const int8_t* bp[4];
    bool aok[2], bok[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int n = n0 + 16 * a + r;
        aok[a] = n < N;
        ap[a] = q + (long)(aok[a] ? n : 0) * K + 16 * g;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int m = m0 + 16 * c + r;
        bok[c] = m < M;
        bp[c] = xq + (long)(bok[c] ? m : 0) * K + 16 * g;
    }
    q8_v4i acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = (q8_v4i){0, 0, 0, 0};
    for (int k0 = 0; k0 < K; k0 += 64) {  // K % 64 == 0: no ragged step
        uint4 A[2], B[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) A[a] = aok[a] ? *reinterpret_cast<const uint4*>(ap[a] + k0) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int c = 0; c < 4; ++c) B[c] = bok[c] ? *reinterpret_cast<const uint4*>(bp[c] + k0) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[a][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const q8_v4i*>(&A[a]), *reinterpret_cast<const q8_v4i*>(&B[c]),
                                                                  acc[a][c], 0, 0, 0);
    }
    // C layout: col (= m) = lane & 15, row (= n) = 4 * (lane >> 4) + reg: a thread owns 8 rows n x 4 rows m. Its 32 outlier sums advance
    // together, column by column in ascending order, so a dequantised weight is formed once per (n, k) and an activation loaded once per (m, k);
    // every sum still sees the operations of q8_epilogue in the same order.
    float o[2][4][4], wsn[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 16 * a + 4 * g + i;
            wsn[a][i] = n < N ? wscale[n] : 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[a][c][i] = 0.0f;
        }
    const int cnt = q8_outlier_count(outliers, K);
    for (int j = 0; j < cnt; ++j) {
        const int k = q8_outlier_col(outliers, j, K);
        float xv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[c] = bok[c] ? bf16_bits_to_f32(x[(long)(m0 + 16 * c + r) * K + k]) : 0.0f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + 16 * a + 4 * g + i;
                const float wdq = n < N ? q8_wdq(q[(long)n * K + k], wsn[a][i]) : 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[a][c][i] = o[a][c][i] + xv[c] * wdq;
            }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + 16 * a + 4 * g + i, m = m0 + 16 * c + r;
                if (m < M && n < N) y[(long)m * N + n] = q8_finish(acc[a][c][i], ascale[m], wsn[a][i], o[a][c][i], res, (long)m * N + n);
            }
}

static bool q8_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

static int q8_check_k(const char* who, int K) {
    if (K % 64 != 0) { set_error("%s: K=%d is not a multiple of 64", who, K); return VAA_E_UNSUPPORTED; }
    if (K > kQ8MaxK) { set_error("%s: K=%d beyond %d (127^2 K must stay below 2^31)", who, K, kQ8MaxK); return VAA_E_UNSUPPORTED; }
    return VAA_OK;
}

}  // namespace vaa

extern "C" int vaa_model_q8_act_quant(const uint16_t* x, int M, int K, float threshold, int8_t* xq, float* ascale, int32_t* outliers, void* stream) {
    using namespace vaa;
    const char* who = "vaa_model_q8_act_quant";
    if (M == 0) return VAA_OK;
    if (!x || !xq || !ascale || !outliers) { set_error("%s: null pointer argument", who); return VAA_E_INVALID; }
    if (M < 1 || K < 64) { set_error("%s: bad sizes (M=%d K=%d)", who, M, K); return VAA_E_INVALID; }
    if (!(threshold >= 0.0f) || !std::isfinite(threshold)) { set_error("%s: the threshold must be finite and >= 0", who); return VAA_E_INVALID; }
    if (const int rc = q8_check_k(who, K)) return rc;
    if (!q8_aligned(x, 16) || !q8_aligned(xq, 16) || !q8_aligned(ascale, 4) || !q8_aligned(outliers, 4)) {
        set_error("%s: x and xq must be 16-byte aligned, ascale and outliers 4-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (M <= kQ8SmallM) {
        VAA_LAUNCH(q8_rows_kernel<false>, dim3((unsigned)M), dim3(kQ8ActThreads), 0, s, x, M, K, threshold, xq, ascale, outliers);
        return check_launch(who);
    }
    const int nv = K / 8;
    VAA_LAUNCH(q8_colflag_kernel, dim3((unsigned)((nv + kQ8FlagCols - 1) / kQ8FlagCols)), dim3(kQ8FlagCols * kQ8FlagRows), 0, s, x, M, K, threshold,
               outliers);
    VAA_LAUNCH(q8_rows_kernel<true>, dim3((unsigned)M), dim3(kQ8ActThreads), 0, s, x, M, K, threshold, xq, ascale, outliers);
    VAA_LAUNCH(q8_compact_kernel, dim3(1), dim3(kQ8ActThreads), 0, s, K, outliers);
    return check_launch(who);
}

extern "C" int vaa_model_q8_matmul(const int8_t* xq, const float* ascale, const int32_t* outliers, const uint16_t* x, int M, const int8_t* q,
                                   const float* wscale, int N, int K, const uint16_t* res, uint16_t* y, int form, void* stream) {
    using namespace vaa;
    const char* who = "vaa_model_q8_matmul";
    if (M == 0) return VAA_OK;
    if (!xq || !ascale || !outliers || !x || !q || !wscale || !y) { set_error("%s: null pointer argument", who); return VAA_E_INVALID; }
    if (M < 1 || N < 1 || K < 64) { set_error("%s: bad sizes (M=%d N=%d K=%d)", who, M, N, K); return VAA_E_INVALID; }
    if (form < 0 || form > 2) { set_error("%s: bad form %d", who, form); return VAA_E_INVALID; }
    if (const int rc = q8_check_k(who, K)) return rc;
    if (form == 1 && M > kQ8SmallM) { set_error("%s: M=%d rows, the split-K form takes at most %d", who, M, kQ8SmallM); return VAA_E_UNSUPPORTED; }
    if (!q8_aligned(xq, 16) || !q8_aligned(x, 16) || !q8_aligned(q, 16) || !q8_aligned(res, 16) || !q8_aligned(y, 16) || !q8_aligned(ascale, 4) ||
        !q8_aligned(wscale, 4) || !q8_aligned(outliers, 4)) {
        set_error("%s: xq, x, q, res and y must be 16-byte aligned, ascale, wscale and outliers 4-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (form == 1 || (form == 0 && M <= kQ8SmallM)) {
        VAA_LAUNCH(q8_gemv_kernel, dim3((unsigned)((N + kQ8GemvRows - 1) / kQ8GemvRows)), dim3(kQ8GemvThreads), 0, s, xq, ascale, outliers, x, M, q,
                   wscale, N, K, res, y);
        return check_launch(who);
    }
    const long gy = ((long)M + kQ8GemmM - 1) / kQ8GemmM;
    if (gy > 65535) { set_error("%s: M=%d beyond the grid", who, M); return VAA_E_UNSUPPORTED; }
    VAA_LAUNCH(q8_gemm_kernel, dim3((unsigned)((N + kQ8GemmN - 1) / kQ8GemmN), (unsigned)gy), dim3(kQ8GemmThreads), 0, s, xq, ascale, outliers, x, M, q,
               wscale, N, K, res, y);
    return check_launch(who);
}
