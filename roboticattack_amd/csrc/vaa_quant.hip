// vaa_quant.hip — the 4-bit block-quantised Llama projections of the evaluation path (include/vaa_model_ops.h: vaa_model_q4_dequant,
// vaa_model_q4_gemv). Inference only. The format (64-element blocks along a row, fp32 absmax per block, two codes per byte with the even
// element in the high nibble, a 16-entry fp32 table passed by the caller) is stated in the header; both kernels form the dequantised weight
// with the ONE device function q4_dequant8 — wq = bf16(table[q] * absmax), one fp32 product (this file is built with -ffp-contract=off),
// rounded to bf16 once — so the prefill route (dequant + stock GEMM) and the decode route (GEMV) see the same model.
//
// vaa_model_q4_dequant: one thread per 16 bytes of codes (32 elements of one block): one 16-byte load, four 16-byte stores. Memory bound.
//
// vaa_model_q4_gemv: y[m, n] = bf16(res[m, n] + sum_k x[m, k] * wq[n, k]) for 1 <= M <= 16 rows of x, on the matrix cores
// (mfma_f32_16x16x32_bf16, A = wq, B = x^T padded to 16 columns with zeros, so C[row n][col m]).
//   * A workgroup of kGemvWaves waves owns kGemvRows = 16 consecutive rows n; the K axis is cut into tiles of kGemvTileK = 128 elements and
//     tile t belongs to wave t % kGemvWaves (one round of the workgroup = one K-chunk of 1024 elements); a wave has two tiles' loads in flight.
//   * In a tile, lane (r = lane & 15, g = lane >> 4) loads the 16 bytes of codes of row n0 + r that hold elements k0 + 32 g .. + 31 (one load
//     instruction covers 64 contiguous bytes of each of the wave's 16 rows; every code byte is read once, by one lane of one workgroup) and
//     the one absmax of their block, and dequantises dword j of the load into the A fragment of MFMA j (j = 0..3). The K slot (g, e) of MFMA j
//     is therefore element k0 + 32 g + 8 j + e; the B fragment follows the same map: lane (m = r, g) loads x[m][k0 + 32 g + 8 j .. + 7], 16
//     bytes per MFMA, 64 contiguous bytes per tile, straight from L2 into the operand registers (x is M * K * 2 <= 352 KB and every workgroup
//     reads all of it; no two waves of a workgroup share a K range, so an LDS copy would serve nobody). Rows m >= M, rows n >= N and the K
//     slots past K of a ragged last tile are zeros that no load touches.
//   * The kGemvWaves partial tiles meet in LDS and are summed in wave order 0 .. kGemvWaves-1 by the thread that then adds res, rounds once
//     and stores y[m, n]. No atomics, no hand-over between workgroups, no waiting on another wave's memory: the same arguments give the same
//     bits, and column m of C depends on column m of B alone, so a row of the result does not depend on the other rows of x.
#include <cmath>

#include "vaa_common.h"
#include "../../include/vaa_model_ops.h"

namespace vaa {

typedef short q4_v8s __attribute__((ext_vector_type(8)));
typedef float q4_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 q4_bf2 __attribute__((ext_vector_type(2)));
typedef float q4_f2 __attribute__((ext_vector_type(2)));

struct Q4Table {
    float v[16];
};

constexpr int kDequantThreads = 256;
constexpr int kGemvWaves = 8, kGemvThreads = 64 * kGemvWaves, kGemvRows = 16, kGemvTileK = 128;  // one round of a workgroup: 1024 elements of K
constexpr int kGemvMaxM = 16;

// two floats -> packed bf16 pair (v_cvt_pk_bf16_f32, round-to-nearest-even)
__device__ __forceinline__ uint32_t q4_cvt_pk_bf16(float lo, float hi) {
    const q4_bf2 r = __builtin_convertvector((q4_f2){lo, hi}, q4_bf2);
    return *reinterpret_cast<const uint32_t*>(&r);
}

// The table into LDS by the first 16 threads (a select chain: no dynamic index into the kernel argument); the caller places the barrier.
__device__ __forceinline__ void q4_fill_table(float* s_tab, const Q4Table& tab, int tid) {
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t = (tid == i) ? tab.v[i] : t;
    if (tid < 16) s_tab[tid] = t;
}

// One dword of codes = 8 consecutive elements (byte b holds element 2b in its high nibble, element 2b+1 in its low nibble) -> 8 bf16 in
// element order. The one source of the dequantised weight: both kernels call it, so their bits agree.
__device__ __forceinline__ uint4 q4_dequant8(uint32_t dw, const float* s_tab, float amax) {
    uint32_t o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t byte = (dw >> (8 * b)) & 0xffu;
        const float even = s_tab[byte >> 4] * amax, odd = s_tab[byte & 15u] * amax;
        o[b] = q4_cvt_pk_bf16(even, odd);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(kDequantThreads) void q4_dequant_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ absmax,
                                                                     const Q4Table tab, long nvec, uint16_t* __restrict__ out) {
    __shared__ float s_tab[16];
    q4_fill_table(s_tab, tab, threadIdx.x);
    __syncthreads();
    const long v = (long)blockIdx.x * kDequantThreads + threadIdx.x;  // 16 bytes of codes = 32 elements = half a block
    if (v >= nvec) return;
    const uint4 c = *reinterpret_cast<const uint4*>(codes + v * 16);
    const float amax = absmax[v >> 1];
    const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(out + v * 32 + j * 8) = q4_dequant8(cw[j], s_tab, amax);
}

struct Q4Tile {
    uint4 c;      // 32 codes of row n0 + r
    float amax;   // their block's absmax
    uint4 xv[4];  // x[m = r][the same 32 elements]
};

// Tile t of the K axis for lane (r, g): zeros (and no load) past the last tile, past K in a ragged last tile, for rows n >= N and m >= M.
__device__ __forceinline__ void q4_load_tile(Q4Tile& q, int t, int tiles, int K, int g, bool wrow, bool xrow, const uint8_t* __restrict__ crow,
                                             const float* __restrict__ arow, const uint16_t* __restrict__ xr) {
    const int k0 = t * kGemvTileK + g * 32;
    const bool live = t < tiles && k0 < K;  // K % 64 == 0 and k0 % 32 == 0: k0 < K means k0 + 32 <= K
    q.c = make_uint4(0u, 0u, 0u, 0u);
    q.amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) q.xv[j] = make_uint4(0u, 0u, 0u, 0u);
    if (live && wrow) {
        q.c = *reinterpret_cast<const uint4*>(crow + k0 / 2);
        q.amax = arow[k0 / 64];
    }
    if (live && xrow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.xv[j] = *reinterpret_cast<const uint4*>(xr + k0 + 8 * j);
    }
}

__device__ __forceinline__ q4_v4f q4_tile_mfma(const Q4Tile& q, const float* s_tab, q4_v4f acc) {
    const uint32_t cw[4] = {q.c.x, q.c.y, q.c.z, q.c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4 a = q4_dequant8(cw[j], s_tab, q.amax);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const q4_v8s*>(&a), *reinterpret_cast<const q4_v8s*>(&q.xv[j]), acc, 0, 0, 0);
    }
    return acc;
}

__global__ __launch_bounds__(kGemvThreads) void q4_gemv_kernel(const uint16_t* __restrict__ x, int M, const uint8_t* __restrict__ codes,
                                                               const float* __restrict__ absmax, const Q4Table tab, int N, int K,
                                                               const uint16_t* __restrict__ res, uint16_t* __restrict__ y) {
    __shared__ float s_tab[16];
    __shared__ float s_acc[kGemvWaves][kGemvMaxM][kGemvRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    q4_fill_table(s_tab, tab, tid);
    __syncthreads();
    const int n0 = blockIdx.x * kGemvRows;
    const bool wrow = n0 + r < N, xrow = r < M;
    const uint8_t* crow = codes + (long)(wrow ? n0 + r : 0) * (K / 2);
    const float* arow = absmax + (long)(wrow ? n0 + r : 0) * (K / 64);
    const uint16_t* xr = x + (long)(xrow ? r : 0) * K;
    const int tiles = (K + kGemvTileK - 1) / kGemvTileK;
    q4_v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = wave; t < tiles; t += 2 * kGemvWaves) {  // two tiles' loads in flight before the first use
        Q4Tile t0, t1;
        q4_load_tile(t0, t, tiles, K, g, wrow, xrow, crow, arow, xr);
        q4_load_tile(t1, t + kGemvWaves, tiles, K, g, wrow, xrow, crow, arow, xr);
        acc = q4_tile_mfma(t0, s_tab, acc);
        acc = q4_tile_mfma(t1, s_tab, acc);
    }
    // C layout: col (= m) = lane & 15, row (= n - n0) = 4 * (lane >> 4) + reg
#pragma unroll
    for (int i = 0; i < 4; ++i) s_acc[wave][r][4 * g + i] = acc[i];
    __syncthreads();
    if (tid < kGemvMaxM * kGemvRows) {
        const int m = tid / kGemvRows, n = n0 + tid % kGemvRows;
        if (m < M && n < N) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < kGemvWaves; ++w) s += s_acc[w][m][tid % kGemvRows];  // the fixed order of the fold over K
            const long at = (long)m * N + n;
            if (res) s += bf16_bits_to_f32(res[at]);
            y[at] = (uint16_t)f32_to_bf16_bits(s);  // the one rounding of y
        }
    }
}

static bool q4_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static Q4Table q4_table(const float* table) {
    Q4Table t;
    for (int i = 0; i < 16; ++i) t.v[i] = table[i];
    return t;
}

}  // namespace vaa

extern "C" int vaa_model_q4_dequant(const uint8_t* codes, const float* absmax, const float* table, int N, int K, uint16_t* out_bf16, void* stream) {
    using namespace vaa;
    const char* who = "vaa_model_q4_dequant";
    if (!codes || !absmax || !table || !out_bf16) { set_error("%s: null pointer argument", who); return VAA_E_INVALID; }
    if (N < 1 || K < 64) { set_error("%s: bad sizes (N=%d K=%d)", who, N, K); return VAA_E_INVALID; }
    if (K % 64 != 0) { set_error("%s: K=%d is not a multiple of the 64-element block", who, K); return VAA_E_UNSUPPORTED; }
    if (!q4_aligned16(codes) || !q4_aligned16(absmax) || !q4_aligned16(out_bf16)) {
        set_error("%s: codes, absmax and out must be 16-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    const long nvec = (long)N * (K / 32);
    const long blocks = (nvec + kDequantThreads - 1) / kDequantThreads;
    if (blocks > 0x7fffffffL) { set_error("%s: N*K beyond the grid", who); return VAA_E_UNSUPPORTED; }
    VAA_LAUNCH(q4_dequant_kernel, dim3((unsigned)blocks), dim3(kDequantThreads), 0, (hipStream_t)stream, codes, absmax, q4_table(table), nvec, out_bf16);
    return check_launch(who);
}

extern "C" int vaa_model_q4_gemv(const uint16_t* x, int M, const uint8_t* codes, const float* absmax, const float* table, int N, int K,
                                 const uint16_t* res, uint16_t* y, void* stream) {
    using namespace vaa;
    const char* who = "vaa_model_q4_gemv";
    if (M == 0) return VAA_OK;
    if (!x || !codes || !absmax || !table || !y) { set_error("%s: null pointer argument", who); return VAA_E_INVALID; }
    if (M < 1 || N < 1 || K < 64) { set_error("%s: bad sizes (M=%d N=%d K=%d)", who, M, N, K); return VAA_E_INVALID; }
    if (K % 64 != 0) { set_error("%s: K=%d is not a multiple of the 64-element block", who, K); return VAA_E_UNSUPPORTED; }
    if (M > kGemvMaxM) { set_error("%s: M=%d rows, at most %d (use vaa_model_q4_dequant and a GEMM)", who, M, kGemvMaxM); return VAA_E_UNSUPPORTED; }
    if (!q4_aligned16(x) || !q4_aligned16(codes) || !q4_aligned16(absmax) || !q4_aligned16(y) || !q4_aligned16(res)) {
        set_error("%s: x, codes, absmax, res and y must be 16-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    const dim3 grid((unsigned)((N + kGemvRows - 1) / kGemvRows)), block(kGemvThreads);
    VAA_LAUNCH(q4_gemv_kernel, grid, block, 0, (hipStream_t)stream, x, M, codes, absmax, q4_table(table), N, K, res, y);
    return check_launch(who);
}
