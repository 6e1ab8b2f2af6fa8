// vaa_decode.hip — single-query attention over a KV cache: one greedy decode step of one Llama layer (include/vaa_model_ops.h:
// vaa_model_attention_decode). Inference only; the training path never comes here.
//
// One launch, one 256-thread workgroup per (head, batch row). A key row of hd bf16 is hd/8 16-byte vectors, so LPK = hd/8 lanes own one key
// and a wave holds 64/LPK keys per load instruction (hd = 128: 4 keys, 1 KiB per wave and instruction). Such a lane group keeps its own
// online-softmax state (running max, running sum, 8 output columns per lane); key j belongs to group j % NG (NG = groups per workgroup), so
// the assignment depends on pos[b] alone. The new key and value never travel through memory: every lane rotates its slice of q and k_new
// with rope_rotate8 (the arithmetic of vaa_model_rope), the first LPK lanes store the rotated k_new and v_new into cache slot pos[b], and the
// group that owns key pos[b] takes it from registers. The NG partial states meet in LDS and are folded in group order 0 .. NG-1 by the hd/8
// threads that then round and store o: no atomics, no hand-over between workgroups, the same bits for the same arguments, and a (b, h)
// pair's result does not depend on what else is in the batch.
//
// The kernel is latency / bandwidth bound (hd = 128, T = 290: 150 KB per workgroup, 2 flop per byte): no MFMA. Each group has KU keys'
// loads (K and V, 2 * KU 16-byte vectors per lane) in flight before the first use.
#include <cmath>

#include "vaa_common.h"
#include "../../include/vaa_model_ops.h"

namespace vaa {

struct DecodeArgs {
    const uint16_t *q, *k_new, *v_new;
    uint16_t *kcache, *vcache, *o;
    const int32_t* pos;
    const float *cos, *sin;  // [Tmax, hd/2]
    unsigned* err_word;
    long q_sb, q_sh, k_sb, k_sh, v_sb, v_sh, o_sb, o_sh;
    long kc_sb, kc_st, kc_sh, vc_sb, vc_st, vc_sh;
    int Tmax;
    float scale_log2;  // softmax scale * log2(e)
};

constexpr int kDecThreads = 256, kDecUnroll = 4;

__device__ __forceinline__ void unpack8_bf16(const uint4& r, float* v) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[2 * q] = __uint_as_float(w[q] << 16); v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
}

// x[c*8 .. c*8+7] of one un-rotated head row after the rotation at position t (c = the lane's vector of the row)
template <int HD>
__device__ __forceinline__ uint4 rotated_vec(const uint16_t* row, const float* cos_t, const float* sin_t, int t, int c) {
    constexpr int HV = HD / 16;  // vectors per half row
    const int cl = c % HV;
    const uint4 lo = *reinterpret_cast<const uint4*>(row + cl * 8), hi = *reinterpret_cast<const uint4*>(row + HD / 2 + cl * 8);
    const float* cp = cos_t + (long)t * (HD / 2) + cl * 8;
    const float* sp = sin_t + (long)t * (HD / 2) + cl * 8;
    const float4 c0 = *reinterpret_cast<const float4*>(cp), c1 = *reinterpret_cast<const float4*>(cp + 4);
    const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
    uint4 ol, oh;
    rope_rotate8(lo, hi, c0, c1, s0, s1, 1.0f, ol, oh);
    return c < HV ? ol : oh;
}

template <int HD>
__global__ __launch_bounds__(kDecThreads) void attention_decode_kernel(const DecodeArgs a) {
    constexpr int LPK = HD / 8;                 // lanes per key row
    constexpr int NG = kDecThreads / LPK;       // key groups per workgroup
    __shared__ float s_m[NG], s_l[NG];
    __shared__ float s_acc[NG][HD];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, c = tid % LPK, gid = tid / LPK;
    const int pos = a.pos[b];
    uint16_t* orow = a.o + (long)b * a.o_sb + (long)h * a.o_sh;
    if (pos < 0 || pos >= a.Tmax) {  // workgroup-uniform: nothing of this row's cache is read or written
        if (tid < LPK) *reinterpret_cast<uint4*>(orow + tid * 8) = make_uint4(0u, 0u, 0u, 0u);
        if (tid == 0 && a.err_word) __hip_atomic_store(a.err_word, VAA_ASYNC_DECODE_POS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // a plain store
        return;
    }
    // this lane's 8 columns of the rotated q, of the rotated new key and of the new value
    const uint4 qv = rotated_vec<HD>(a.q + (long)b * a.q_sb + (long)h * a.q_sh, a.cos, a.sin, pos, c);
    const uint4 knv = rotated_vec<HD>(a.k_new + (long)b * a.k_sb + (long)h * a.k_sh, a.cos, a.sin, pos, c);
    const uint4 vnv = *reinterpret_cast<const uint4*>(a.v_new + (long)b * a.v_sb + (long)h * a.v_sh + c * 8);
    uint16_t* kc = a.kcache + (long)b * a.kc_sb + (long)h * a.kc_sh;
    uint16_t* vc = a.vcache + (long)b * a.vc_sb + (long)h * a.vc_sh;
    if (tid < LPK) {  // cache slot pos: written here, read by nobody in this launch (keys < pos come from the cache, key pos from registers)
        *reinterpret_cast<uint4*>(kc + (long)pos * a.kc_st + c * 8) = knv;
        *reinterpret_cast<uint4*>(vc + (long)pos * a.vc_st + c * 8) = vnv;
    }
    float qf[8];
    unpack8_bf16(qv, qf);

    float m = -INFINITY, l = 0.0f, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j0 = gid; j0 <= pos; j0 += NG * kDecUnroll) {
        uint4 kv[kDecUnroll], vv[kDecUnroll];
#pragma unroll
        for (int u = 0; u < kDecUnroll; ++u) {  // every load of the batch before the first use
            const int j = j0 + u * NG;
            if (j < pos) {
                kv[u] = *reinterpret_cast<const uint4*>(kc + (long)j * a.kc_st + c * 8);
                vv[u] = *reinterpret_cast<const uint4*>(vc + (long)j * a.vc_st + c * 8);
            } else {
                kv[u] = knv;
                vv[u] = vnv;
            }
        }
#pragma unroll
        for (int u = 0; u < kDecUnroll; ++u) {
            const int j = j0 + u * NG;  // the same for the LPK lanes of a group
            float kf[8], vf[8];
            unpack8_bf16(kv[u], kf);
            unpack8_bf16(vv[u], vf);
            float s = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s = __builtin_fmaf(qf[e], kf[e], s);
#pragma unroll
            for (int off = 1; off < LPK; off <<= 1) s += __shfl_xor(s, off, 64);  // butterfly: every lane of the group ends with the same bits
            if (j <= pos) {
                const float mn = fmaxf(m, s);  // the running max of the raw dot products (scale > 0: max commutes with the scaling)
                const float alpha = __builtin_amdgcn_exp2f((m - mn) * a.scale_log2);  // m = -inf -> 0
                const float p = __builtin_amdgcn_exp2f((s - mn) * a.scale_log2);
                l = __builtin_fmaf(l, alpha, p);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(acc[e], alpha, p * vf[e]);
                m = mn;
            }
        }
    }
    if (c == 0) { s_m[gid] = m; s_l[gid] = l; }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[gid][c * 8 + e] = acc[e];
    __syncthreads();
    if (tid < LPK) {  // fold the NG states in group order; thread tid owns columns tid*8 .. tid*8+7
        float M = -INFINITY;
        for (int g = 0; g < NG; ++g) M = fmaxf(M, s_m[g]);  // finite: key pos exists
        float L = 0.0f, out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int g = 0; g < NG; ++g) {
            const float mg = s_m[g];
            if (mg == -INFINITY) continue;  // a group without keys
            const float w = __builtin_amdgcn_exp2f((mg - M) * a.scale_log2);
            L = __builtin_fmaf(s_l[g], w, L);
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] = __builtin_fmaf(s_acc[g][tid * 8 + e], w, out[e]);
        }
        uint32_t pk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pk[q] = f32_to_bf16_bits(out[2 * q] / L) | (f32_to_bf16_bits(out[2 * q + 1] / L) << 16);  // the one rounding of o
        *reinterpret_cast<uint4*>(orow + tid * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace vaa

extern "C" int vaa_model_attention_decode(const uint16_t* q, const int64_t* q_str, const uint16_t* k_new, const int64_t* k_str, const uint16_t* v_new,
                                          const int64_t* v_str, uint16_t* kcache, const int64_t* kc_str, uint16_t* vcache, const int64_t* vc_str,
                                          const int32_t* pos, const float* cos_t, const float* sin_t, uint16_t* o, const int64_t* o_str, int B, int H,
                                          int Tmax, int hd, float scale, void* stream) {
    using namespace vaa;
    const char* who = "vaa_model_attention_decode";
    if (B == 0) return VAA_OK;
    const void* ptrs[] = {q, q_str, k_new, k_str, v_new, v_str, kcache, kc_str, vcache, vc_str, pos, cos_t, sin_t, o, o_str};
    const char* names[] = {"q", "q_str", "k_new", "k_str", "v_new", "v_str", "kcache", "kc_str", "vcache", "vc_str", "pos", "cos", "sin", "o", "o_str"};
    for (int i = 0; i < 15; ++i)
        if (!ptrs[i]) { set_error("%s: null pointer argument (%s)", who, names[i]); return VAA_E_INVALID; }
    if (B < 0 || H <= 0 || Tmax <= 0) { set_error("%s: bad sizes (B=%d H=%d Tmax=%d)", who, B, H, Tmax); return VAA_E_INVALID; }
    if (!std::isfinite(scale) || !(scale > 0.0f)) { set_error("%s: scale must be finite and > 0 (scale=%g)", who, (double)scale); return VAA_E_INVALID; }
    if (hd != 128 && hd != 16) { set_error("%s: head width %d is not supported (128 or 16)", who, hd); return VAA_E_UNSUPPORTED; }
    if (B > 65535) { set_error("%s: B=%d beyond the grid's second dimension", who, B); return VAA_E_UNSUPPORTED; }
    // 16-byte vector accesses: every base and every stride a multiple of 8 elements
    const int64_t strs[] = {q_str[0], q_str[1], k_str[0], k_str[1], v_str[0], v_str[1], o_str[0], o_str[1],
                            kc_str[0], kc_str[1], kc_str[2], vc_str[0], vc_str[1], vc_str[2]};
    for (int i = 0; i < 14; ++i)
        if (strs[i] % 8 != 0) { set_error("%s: every stride must be a multiple of 8 elements (got %lld)", who, (long long)strs[i]); return VAA_E_UNSUPPORTED; }
    if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) || !aligned16(kcache) || !aligned16(vcache) || !aligned16(o) || !aligned16(cos_t) ||
        !aligned16(sin_t)) {
        set_error("%s: q, k_new, v_new, kcache, vcache, o, cos and sin must be 16-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    DecodeArgs a;
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.kcache = kcache; a.vcache = vcache; a.o = o; a.pos = pos; a.cos = cos_t; a.sin = sin_t;
    a.err_word = async_error_word();
    a.q_sb = q_str[0]; a.q_sh = q_str[1]; a.k_sb = k_str[0]; a.k_sh = k_str[1]; a.v_sb = v_str[0]; a.v_sh = v_str[1]; a.o_sb = o_str[0]; a.o_sh = o_str[1];
    a.kc_sb = kc_str[0]; a.kc_st = kc_str[1]; a.kc_sh = kc_str[2]; a.vc_sb = vc_str[0]; a.vc_st = vc_str[1]; a.vc_sh = vc_str[2];
    a.Tmax = Tmax;
    a.scale_log2 = scale * 1.4426950408889634f;
    const dim3 grid((unsigned)H, (unsigned)B), block(kDecThreads);
    if (hd == 128) VAA_LAUNCH(attention_decode_kernel<128>, grid, block, 0, (hipStream_t)stream, a);
    else VAA_LAUNCH(attention_decode_kernel<16>, grid, block, 0, (hipStream_t)stream, a);
    return check_launch(who);
}
