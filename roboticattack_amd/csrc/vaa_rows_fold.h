// vaa_rows_fold.h — the device primitives of the K3 loss family and the fold of its per-row statistics into the loss scalars, shared by
// vaa_loss.hip (K3, the step epilogue), vaa_head.hip (K3h's finishing launch) and vaa_head_slice.hip (K3s: the slice-only LM head that folds
// inside its own launch). The forms of the family are bit-equal because each piece of arithmetic is written here once.
#pragma once
#include <math.h>

#include "vaa_common.h"
#include "vaa_rows.h"

namespace vaa {

struct RowStat {  // one per LABELLED row, stored compactly at its row-major rank `rowidx` among labelled positions
    float lse;   // logsumexp over all V classes
    float zlab;  // logit of the label
    float alse;  // logsumexp over the 256 action classes
    float E;     // sum_a softmax_a * (a+1), in [1,256]
    int pred;    // 31744 + argmax over the action slice
    int pos;     // position p = b*(L-1)+k
    int lab;     // the label (token id)
    int ord;     // rank of this position among its sample's labelled positions (0 = first)
    int predf;   // argmax over ALL V classes (lowest index on ties, torch.argmax)
};

__device__ __forceinline__ double bin_center(int tok) {  // ActionTokenizer.decode_token_ids_to_actions (action_tokenizer.py:49-68)
    int d = 32000 - tok - 1;
    d = d < 0 ? 0 : (d > 254 ? 254 : d);
    return -1.0 + (2.0 * d + 1.0) / 255.0;
}

// 16 bytes of logits <-> fp32 registers
template <typename T>
struct Vec;
template <>
struct Vec<float> {
    static constexpr int N = 4;
    __device__ static void load(const float* p, float* v) {
        float4 r = *reinterpret_cast<const float4*>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
    __device__ static void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    __device__ static float get(const float* p) { return *p; }
};
template <>
struct Vec<uint16_t> {  // bf16 bits
    static constexpr int N = 8;
    __device__ static void load(const uint16_t* p, float* v) {
        uint4 r = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[2 * q] = __uint_as_float(w[q] << 16); v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
    }
    __device__ static void store(uint16_t* p, const float* v) {
        uint4 r;
        r.x = f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16);
        r.y = f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16);
        r.z = f32_to_bf16_bits(v[4]) | (f32_to_bf16_bits(v[5]) << 16);
        r.w = f32_to_bf16_bits(v[6]) | (f32_to_bf16_bits(v[7]) << 16);
        *reinterpret_cast<uint4*>(p) = r;
    }
    __device__ static float get(const uint16_t* p) { return bf16_bits_to_f32(*p); }
};

// neutral element of the combination of a row's parts (row_lse): "no full-vocabulary statistics"
__device__ __forceinline__ PartStat neutral_part() {
    PartStat p;
    p.m = -INFINITY; p.s = 0.0f; p.zlab = -INFINITY; p.amax = 0x7fffffff;
    return p;
}

// maximum with its index over a wave, lowest index on ties (torch.argmax); every lane gets the result
__device__ __forceinline__ void wave_argmax(float& m, int& mi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
}
// ... and over a workgroup of NT threads: waves through LDS, combined in wave order by every thread. `z` (with its own LDS words `redz`) is
// max-reduced on the way when given. No barrier follows the combination: a caller that writes the LDS words again (a next row, another
// reduction through the same words) puts its own barrier in front of that write.
template <int NT>
__device__ __forceinline__ void block_argmax(float& m, int& mi, float* redm, int* redi, float* z = nullptr, float* redz = nullptr) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    wave_argmax(m, mi);
    if (z) *z = wave_max(*z);
    if (lane == 0) {
        redm[wv] = m; redi[wv] = mi;
        if (z) redz[wv] = *z;
    }
    __syncthreads();
    m = redm[0]; mi = redi[0];
    if (z) *z = redz[0];
    for (int q = 1; q < NT / 64; ++q) {
        if (redm[q] > m || (redm[q] == m && redi[q] < mi)) { m = redm[q]; mi = redi[q]; }
        if (z) *z = fmaxf(*z, redz[q]);
    }
}

// Soft-argmax statistics of the 256 action logits by ONE wave (UADA.py:384-389, UPA.py:370-374): lane l holds the N logits of columns
// [l N, l N + N), -inf in lanes that own none. alse = log-sum-exp over the slice, E = sum_a softmax_a (a + 1), pred = kA0 + argmax.
template <int N>
__device__ __forceinline__ void slice_soft_argmax(const float (&x)[N], float& alse, float& E, int& pred) {
    const int lane = threadIdx.x & 63;
    int ai = 0;
#pragma unroll
    for (int e = 1; e < N; ++e) if (x[e] > x[ai]) ai = e;
    float bestv = x[ai], am = x[ai];  // (the lane maximum IS x[ai])
    int besti = lane * N + ai;
    wave_argmax(bestv, besti);
    am = wave_max(am);
    float es = 0.0f, ew = 0.0f;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const float ex = expf(x[e] - am);
        es += ex;
        ew += ex * (float)(lane * N + e + 1);
    }
    es = wave_sum(es);
    ew = wave_sum(ew);
    alse = am + logf(es);
    E = ew / es;
    pred = kA0 + besti;
}

// d [w^2 mean((E / 256 - t)^2)] / d E of one action row (UADA.py:390-394; A-D10: the target 1/256 -> 0), nact = rows the mean runs over
// (an int count or a folded double: converted where it divides)
template <typename C>
__device__ __forceinline__ float mse_kE(float w, float E, int lab, C nact) {
    const double q = (double)E / 256.0, t = (lab > 31872) ? 0.0 : 1.0;
    return (float)((double)w * w * 2.0 * (q - t) / nact / 256.0);
}
// d E / d z of action bin a (0-based) times kE: kE p_a ((a + 1) - E)
__device__ __forceinline__ float slice_grad(float z, int a, float kE, float alse, float E) { return kE * expf(z - alse) * ((float)(a + 1) - E); }
// d total / d z of the logit in column `col` of a row: kce (softmax - onehot), plus the slice term in the action columns
__device__ __forceinline__ float logit_grad(float z, int col, int lab, float kce, float lse, bool in_slice, float kE, float alse, float E) {
    float gv = 0.0f;
    if (kce != 0.0f) gv = kce * (expf(z - lse) - (col == lab ? 1.0f : 0.0f));
    if (in_slice && kE != 0.0f) gv += slice_grad(z, col - kA0, kE, alse, E);
    return gv;
}

// block-wide sums of NV doubles at once (fixed order: lanes by xor-shuffle, then waves 0..15) -> deterministic
template <int NV, int NT = 1024>
__device__ __forceinline__ void block_sums(double (&v)[NV], double (*sh)[NV]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) sh[wv][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double t = 0.0;
        for (int w = 0; w < NT / 64; ++w) t += sh[w][q];
        v[q] = t;
    }
}

// UPA per-sample terms from the E / label of a sample's first three labelled rows (UPA.py:375-384)
struct Upa3 {
    double e[3], l[3];
    __device__ void set(int q, const RowStat& s) { e[q] = ((double)s.E - 1.0) / 255.0; l[q] = ((double)(s.lab - 31743) - 1.0) / 255.0; }
    __device__ void terms(double& cosp1, double& nd) const {
        const double dot = e[0] * l[0] + e[1] * l[1] + e[2] * l[2];
        const double ne = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], nl = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
        const double d0 = e[0] - l[0], d1 = e[1] - l[1], d2 = e[2] - l[2];
        cosp1 = dot / (fmax(sqrt(ne), 1e-8) * fmax(sqrt(nl), 1e-8)) + 1.0;  // F.cosine_similarity + 1 (UPA.py:382-383)
        nd = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    }
    __device__ double dE(int q, double alpha, double beta, double aux1, int B) const {  // d total / d e[q]
        const double dot = e[0] * l[0] + e[1] * l[1] + e[2] * l[2];
        const double ne = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], nl = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
        const double d0 = e[0] - l[0], d1 = e[1] - l[1], d2 = e[2] - l[2];
        const double sne = fmax(sqrt(ne), 1e-8), snl = fmax(sqrt(nl), 1e-8), nd = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double eq = q == 0 ? e[0] : (q == 1 ? e[1] : e[2]), lq = q == 0 ? l[0] : (q == 1 ? l[1] : l[2]);
        const double dcos = lq / (sne * snl) - dot * eq / (sne * sne * sne * snl);
        const double dn = nd > 0 ? (eq - lq) / nd : 0.0;
        return alpha * dcos / B - beta * aux1 * aux1 * dn / B;
    }
};

struct RowsArgs {
    const void* logits;
    const int* rowmap;  // hdr[4] + RowMap[R]
    PartStat* part;     // [R][split]
    SliceStat* slice;   // [R]
    void* grad;
    float* scalars;
    int32_t* pred_tokens;
    int32_t* pred_full;
    int R, B, L, V, mode, split, grad_slice;
    int ldz, zcol0;     // logits row stride (elements) and the vocabulary column of its first element: V, 0 — or 256, kA0 when `logits` is the
                        // action-column buffer vaa_head_loss_rows_stats left (vaa_head_loss_rows_finish: only the slice is ever read)
    float w, alpha, beta, scale;
};

// Group g's view of a call over P groups (a segmented map, or an ordinary map with P = 1): its own map, its rows of the statistics, its
// images of the prediction maps, its scalars[8g..] — what a standalone call on the group alone is handed, so rows_fold on it folds those bits.
__device__ __forceinline__ RowsArgs rows_group_view(const RowsArgs& a, int P, int g) {
    RowsArgs ag = a;
    const int* map = a.rowmap;
    const int Pm = map[2], Bp = a.B / P;
    const bool total_ok = map[0] == a.R && (Pm == P || (Pm == 0 && P == 1));
    int r0 = 0;
    if (Pm > 0 && g < Pm) {
        r0 = map[rowmap_seg_table(a.B, a.L) + 4 * g];
        ag.rowmap = map + rowmap_seg_sub(a.B, a.L, Pm, g);
    }
    ag.R = total_ok ? ag.rowmap[0] : -1;  // a map of another batch than the caller states: rows_fold publishes NaN and never reads it
    ag.B = Bp;
    ag.part = a.part + (size_t)r0 * a.split;
    ag.slice = a.slice + r0;
    ag.scalars = a.scalars + 8 * g;
    if (a.pred_tokens) ag.pred_tokens = a.pred_tokens + (size_t)g * Bp * (a.L - 1);
    if (a.pred_full) ag.pred_full = a.pred_full + (size_t)g * Bp * (a.L - 1);
    return ag;
}

struct FoldOut {
    double nrow, nact, CE, MSE, UAD, total, aux0, aux1, dce;
    int Rn;
};
// one-pass hand-over (rows_stats_kernel<.., true>): the folding workgroup leaves every row's log-sum-exp beside its slice statistics
// (SliceStat::pad) and publishes what every gradient needs as two SELF-VALIDATING 64-bit words {generation, payload} — a waiting workgroup
// polls exactly those two words and needs no ordering between them — BEFORE it writes the scalars and prediction maps nobody waits for
struct Handover {
    unsigned long long* words;  // [0] = {gen, bits of kce = dce / nrow as fp32}, [1] = {gen, nact | Rn << 16}
    unsigned gen;
};
template <int kRowsT, bool COH = false>
__device__ __forceinline__ FoldOut rows_fold(const RowsArgs& a, bool publish, double (*sh)[7], Handover ho = Handover{nullptr, 0u});

// statistics words another workgroup of the SAME launch wrote: agent-scope atomics go past the per-XCD L2 (COH); plain accesses otherwise
template <bool COH, typename S>
__device__ __forceinline__ S stat_load(const S* p) {
    static_assert(sizeof(S) == 16, "four words");
    if (!COH) return *p;
    unsigned w[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) w[z] = __hip_atomic_load(reinterpret_cast<const unsigned*>(p) + z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S v;
    __builtin_memcpy(&v, w, 16);
    return v;
}
template <bool COH, typename S>
__device__ __forceinline__ void stat_store(S* p, const S& v) {
    static_assert(sizeof(S) == 16, "four words");
    if (!COH) { *p = v; return; }
    unsigned w[4];
    __builtin_memcpy(w, &v, 16);
#pragma unroll
    for (int z = 0; z < 4; ++z) __hip_atomic_store(reinterpret_cast<unsigned*>(p) + z, w[z], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Combines the `split` parts of row rr: returns its log-sum-exp, with the label's logit and the full-vocabulary argmax (lowest index on ties)
template <bool COH>
__device__ __forceinline__ float row_lse(const PartStat* part, int split, int rr, float& zlab, int& amax) {
    float M = -INFINITY, tot = 0.0f, best = -INFINITY;
    zlab = -INFINITY;
    amax = 0x7fffffff;
    constexpr int kHeld = 8;
    if (COH && split <= kHeld) {  // coherent loads are not merged by the compiler: fetch every part ONCE, all requests in flight together
        PartStat ps[kHeld];
#pragma unroll
        for (int q = 0; q < kHeld; ++q)
            if (q < split) ps[q] = stat_load<COH>(&part[(size_t)rr * split + q]);
#pragma unroll
        for (int q = 0; q < kHeld; ++q)
            if (q < split) M = fmaxf(M, ps[q].m);
#pragma unroll
        for (int q = 0; q < kHeld; ++q)
            if (q < split) {
                tot += ps[q].s * expf(ps[q].m - M);
                zlab = fmaxf(zlab, ps[q].zlab);
                if (ps[q].m > best || (ps[q].m == best && ps[q].amax < amax)) { best = ps[q].m; amax = ps[q].amax; }
            }
        if (M == -INFINITY) { zlab = 0.0f; amax = -1; return 0.0f; }  // every part neutral: a slice-only step (see below)
        return M + logf(tot);
    }
    for (int q = 0; q < split; ++q) M = fmaxf(M, stat_load<COH>(&part[(size_t)rr * split + q]).m);
    for (int q = 0; q < split; ++q) {
        const PartStat p = stat_load<COH>(&part[(size_t)rr * split + q]);
        tot += p.s * expf(p.m - M);
        zlab = fmaxf(zlab, p.zlab);
        if (p.m > best || (p.m == best && p.amax < amax)) { best = p.m; amax = p.amax; }
    }
    // every part neutral {m = -inf, s = 0}: the row has NO full-vocabulary statistics — a slice-only step (vaa_head_slice_fwd_bwd: the loop
    // reads CE / the full argmax on 1 of innerLoop steps, UADA_ddp.py:214-221, and never in UPA's reverse-direction mode, UPA.py:145-186).
    // The row then adds 0 to CE and -1 to pred_full; real logits never have a maximum of -inf
    if (M == -INFINITY) { zlab = 0.0f; amax = -1; return 0.0f; }
    return M + logf(tot);
}
// the E / label of the three consecutive rows r0.. (a sample's first three labelled rows)
template <bool COH>
__device__ __forceinline__ Upa3 upa_load(const SliceStat* slice, const RowMap* rm, int r0) {
    Upa3 u;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        RowStat t;
        t.E = stat_load<COH>(&slice[r0 + q]).E;
        t.lab = rm[r0 + q].lab;
        u.set(q, t);
    }
    return u;
}

// Folds the R compact row statistics into the loss scalars in a fixed order (thread t takes rows t, t + kRowsT, ...; block_sums), and — for
// the publishing workgroup — writes scalars[8] and the two prediction maps. Shared by rows_finish_kernel and the step epilogue.
template <int kRowsT, bool COH>
__device__ __forceinline__ FoldOut rows_fold(const RowsArgs& a, bool publish, double (*sh)[7], Handover ho) {
    const int tid = threadIdx.x;
    const RowMap* rm = reinterpret_cast<const RowMap*>(a.rowmap + 4);
    const int Rdev = a.rowmap[0];
    const int Rn = min(a.R, Rdev);  // rows both the caller and the map know: a mismatch publishes NaN and never leaves the map
    const bool handing = COH && ho.words != nullptr;
    auto clear_maps = [&]() {
        const int P0 = a.B * (a.L - 1);
        if (a.pred_tokens) for (int q = tid; q < P0; q += kRowsT) a.pred_tokens[q] = -1;
        if (a.pred_full) for (int q = tid; q < P0; q += kRowsT) a.pred_full[q] = -1;
    };
    // the publishing workgroup clears the prediction maps NOW, under the statistics' load latency (the barriers of the block reduction below
    // order these stores before the per-row stores that follow it) — unless a grid is waiting for this fold: then nothing is queued in front
    // of the statistics loads and the maps are cleared after the hand-over
    if (publish && !handing) clear_maps();
    int first_am = 0;  // full-vocabulary argmax of this thread's first row (rr = tid), kept for the publication
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};  // ce, mse, uad, nrow, nact, upa sum(cos+1), upa sum ||e'-l'||
    for (int rr = tid; rr < Rn; rr += kRowsT) {
        const RowMap m = rm[rr];
        float zl;
        int am;
        SliceStat ss_early = {0.f, 0.f, 0, 0};
        if (handing) ss_early = stat_load<COH>(&a.slice[rr]);  // requested together with the parts: one round trip for the whole row
        const float lse = row_lse<COH>(a.part, a.split, rr, zl, am);
        if (handing)  // the row's workgroups take their log-sum-exp from here instead of combining the parts again
            __hip_atomic_store(reinterpret_cast<unsigned*>(&a.slice[rr].pad), __float_as_uint(lse), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rr == tid) first_am = am;
        acc[3] += 1.0;
        acc[0] += (double)lse - (double)zl;
        if (m.lab > 2) {
            const SliceStat ss = handing ? ss_early : stat_load<COH>(&a.slice[rr]);
            acc[4] += 1.0;
            const double q = (double)ss.E / 256.0, t = (m.lab > 31872) ? 0.0 : 1.0;  // UADA.py:390-394 (A-D10: 1/256 -> 0)
            acc[1] += (q - t) * (q - t);
            const double ag = bin_center(m.lab), ap = bin_center(ss.pred);  // cal_UAD, UADA.py:408-418
            acc[2] += fabs(ap - ag) / (ag > 0 ? fabs(ag + 1.0) : fabs(ag - 1.0));
        }
        if (a.mode == VAA_LOSS_UPA && m.ord == 0 && rr + 2 < Rn) {  // first three labelled rows of a sample are consecutive ranks
            const Upa3 u = upa_load<COH>(a.slice, rm, rr);
            double c1, nd;
            u.terms(c1, nd);
            acc[5] += c1;
            acc[6] += nd;
        }
    }
    block_sums<7, kRowsT>(acc, sh);
    FoldOut f;
    f.Rn = Rn;
    f.nrow = acc[3]; f.nact = acc[4];
    f.CE = f.nrow > 0 ? acc[0] / f.nrow : 0.0;
    f.MSE = f.nact > 0 ? (double)a.w * a.w * acc[1] / f.nact : 0.0;
    f.UAD = f.nact > 0 ? acc[2] / f.nact : 0.0;
    f.total = 0.0; f.aux0 = 0.0; f.aux1 = 0.0; f.dce = 0.0;
    if (a.mode == VAA_LOSS_UPA) {
        f.aux0 = acc[5] / a.B;
        f.aux1 = 1.0 / (acc[6] / a.B + 1e-3);  // UPA.py:384
        f.total = (double)a.alpha * f.aux0 + (double)a.beta * f.aux1;
    } else if (a.mode == VAA_LOSS_UADA) { f.total = f.MSE + 1.0 / f.CE; f.dce = -1.0 / (f.CE * f.CE); }  // UADA.py:147
    else if (a.mode == VAA_LOSS_UADA_DDP) { f.total = f.MSE; }                                           // UADA_ddp.py:203-206
    else { f.total = (double)a.scale * f.CE; f.dce = (double)a.scale; }                                 // TMA.py:148
    if (handing) {  // the waiting workgroups need {kce, nact, Rn}: hand over now, publish afterwards
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this thread's log-sum-exp words have COMPLETED before the publication below
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        if (tid == 0) {
            const float kce = f.nrow > 0 ? (float)(f.dce / f.nrow) : 0.0f;
            const unsigned long long g = (unsigned long long)ho.gen << 32;
            __hip_atomic_store(&ho.words[0], g | __float_as_uint(kce), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ho.words[1], g | ((unsigned)f.nact & 0xffffu) | ((unsigned)f.Rn << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (publish && handing) {
        clear_maps();
        __syncthreads();
    }
    if (publish) {
        if (tid == 0) {
            const bool ok = Rdev == a.R;  // the caller's row count must be the row map's
            a.scalars[0] = ok ? (float)f.total : __uint_as_float(0x7fc00000u);
            a.scalars[1] = (float)f.CE; a.scalars[2] = (float)f.MSE; a.scalars[3] = (float)f.aux0;
            a.scalars[4] = (float)f.aux1; a.scalars[5] = (float)f.nrow; a.scalars[6] = (float)f.nact; a.scalars[7] = (float)f.UAD;
        }
        for (int rr = tid; rr < Rn; rr += kRowsT) {
            const RowMap m = rm[rr];
            const int pos = m.b * (a.L - 1) + m.k;
            if ((unsigned)pos >= (unsigned)(a.B * (a.L - 1))) continue;  // a map built for other sizes than the caller states
            if (a.pred_tokens && m.lab > 2) a.pred_tokens[pos] = stat_load<COH>(&a.slice[rr]).pred;
            if (a.pred_full) {
                int am = first_am;
                if (rr != tid) {  // more rows than threads: combine the parts again
                    float zl;
                    row_lse<COH>(a.part, a.split, rr, zl, am);
                }
                a.pred_full[pos] = am;
            }
        }
    }
    return f;
}

// At most ONE stream of the process has grids in flight whose workgroups wait for each other (vaa_loss.hip's one-pass K3, vaa_head_slice.hip's K3s):
// a request from another stream is admitted only once the owner stream has drained — two half-resident waiting grids would otherwise be possible.
bool rows_one_pass_stream_ok(hipStream_t st);

}  // namespace vaa
