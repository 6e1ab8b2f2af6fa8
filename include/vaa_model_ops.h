/*
 * vaa_model_ops.h — OPTIONAL fused elementwise operators for the PyTorch-ROCm model that surrounds the hot path
 * (same libvaa_hip.so, same conventions as vaa.h). They are NOT part of the reference's interface nor of the SURVEY.md
 * section-8 contract; the model runs without them (VAA_NO_FUSED_MODEL_OPS=1).
 */
#ifndef VAA_MODEL_OPS_H_
#define VAA_MODEL_OPS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* HF rotate_half rotary embedding on bf16 x[B,T,H,hd] (element strides sb,st,sh; last dim contiguous) -> contiguous out.
 * cos_t/sin_t: float32 [T,hd/2]. sin_sign = +1 forward, -1 backward (the adjoint is the inverse rotation). */
int vaa_model_rope(const uint16_t* x, long sb, long st, long sh, const float* cos_t, const float* sin_t, int B, int T, int H, int hd,
                   float sin_sign, uint16_t* out, void* stream);
/* y = silu(gate) * up over n contiguous bf16 elements (n % 8 == 0), and its backward. */
int vaa_model_swiglu_fwd(const uint16_t* gate, const uint16_t* up, uint16_t* y, long n, void* stream);
int vaa_model_swiglu_bwd(const uint16_t* dy, const uint16_t* gate, const uint16_t* up, uint16_t* dgate, uint16_t* dup, long n, void* stream);
/* LayerScale + residual: out[r, :] = x[r, :] + a[r, :] * ls (ls bf16 [D], D % 8 == 0; x may be NULL: out = a * ls). */
int vaa_model_scale_add(const uint16_t* x, const uint16_t* a, const uint16_t* ls, uint16_t* out, long rows, int D, void* stream);
/* RMSNorm over rows of D bf16 (weight bf16 [D], HF LlamaRMSNorm rounding) saving rstd float32 [rows]; the backward adds the
 * residual pass-through gradient gpass (may be NULL): gx = gpass + rstd*(gh*w - xhat*mean(gh*w*xhat)). */
int vaa_model_rmsnorm_fwd(const uint16_t* x, const uint16_t* w, uint16_t* h, float* rstd, long rows, int D, float eps, void* stream);
int vaa_model_rmsnorm_bwd(const uint16_t* gh, const uint16_t* gpass, const uint16_t* x, const uint16_t* w, const float* rstd, uint16_t* gx,
                          long rows, int D, void* stream);
/* LayerNorm over rows of D bf16 (weight, bias bf16 [D]; fp32 statistics, one rounding) saving {mean, rstd} float32 [rows,2]; the
 * backward adds the residual pass-through gradient gpass (may be NULL). Weight and bias are frozen (no gradients). */
int vaa_model_layernorm_fwd(const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* h, float* stats, long rows, int D, float eps,
                            void* stream);
int vaa_model_layernorm_bwd(const uint16_t* gh, const uint16_t* gpass, const uint16_t* x, const uint16_t* w, const float* stats, uint16_t* gx,
                            long rows, int D, void* stream);
/* Softmax attention on the matrix cores for short sequences. q,k,v,o: bf16 views [B,T,H,hd] given by element strides
 * {batch, token, head} (last dim contiguous, all strides % 8 == 0), hd % 8 == 0, hd <= 128. lse: float32 [B,H,T] (natural log).
 * causal != 0: query t sees keys <= t.
 * 32-bit range: a (batch, head) slice is addressed with 32-bit byte counts and offsets, so for every operand the token stride must be
 * >= 0 and ((T-1)*stride_t + hd)*2 as well as ((roundup(T,64)-1)*stride_t + padded hd)*2 (padded hd = 64 / 96 / 128) must be <= 2^31-1.
 * scale must be finite and > 0 (the running max is taken before the scaling). Either violation returns VAA_E_UNSUPPORTED before any launch;
 * both hold for vaa_model_attention_bwd too.
 * cu_seqlens (int32 [B+1], may be NULL): the B sequences are PACKED back to back along the token axis (the batch stride is unused),
 * sample b owning tokens cu[b] .. cu[b+1]-1; T is then the maximum length (lse and dsum stay [B,H,T]). */
int vaa_model_attention_fwd(const uint16_t* q, const int64_t* q_str, const uint16_t* k, const int64_t* k_str, const uint16_t* v,
                            const int64_t* v_str, uint16_t* o, const int64_t* o_str, float* lse, const int32_t* cu_seqlens, int B, int H,
                            int T, int hd, int causal, float scale, void* stream);
/* Backward of vaa_model_attention_fwd: o, lse from the forward; dsum: float32 [B,H,T] workspace; dq/dk/dv: bf16 [B,T,H,hd] views
 * given by strides (e.g. the three slices of one packed [B,T,3,H,hd] gradient buffer). Two launches (dq, then dk/dv).
 * rope_cos/rope_sin (both or neither; float32 [T,hd/2], hd in {64,128}): q and k had vaa_model_rope applied before the forward;
 * dq and dk are then returned w.r.t. the un-rotated tensors (the adjoint rotation runs in the kernels' epilogues); with cu_seqlens the
 * tables are indexed by the PACKED token (one row per token, i.e. already gathered by position id). */
int vaa_model_attention_bwd(const uint16_t* q, const int64_t* q_str, const uint16_t* k, const int64_t* k_str, const uint16_t* v,
                            const int64_t* v_str, const uint16_t* o, const int64_t* o_str, const uint16_t* dout, const int64_t* do_str,
                            const float* lse, float* dsum, uint16_t* dq, const int64_t* dq_str, uint16_t* dk, const int64_t* dk_str,
                            uint16_t* dv, const int64_t* dv_str, const float* rope_cos, const float* rope_sin, const int32_t* cu_seqlens, int B,
                            int H, int T, int hd, int causal, float scale, void* stream);
/* One greedy decode step of one Llama layer: single-query softmax attention over a KV cache, for all B rows in ONE launch (inference only).
 * Arguments
 *   q, k_new, v_new  bf16 [B,H,hd] views, UN-rotated, given by element strides {batch, head} (e.g. the three slices of the step's packed
 *                    QKV GEMM output [B,3,H,hd]); last dim contiguous.
 *   kcache, vcache   bf16 [B,Tmax,H,hd] views given by element strides {batch, token, head}; read AND written.
 *   pos              device int32 [B]: row b's current position (its cache holds keys 0 .. pos[b]-1); rows may differ.
 *   cos_t, sin_t     float32 [Tmax, hd/2], the tables vaa_model_rope takes.
 *   o                bf16 [B,H,hd] view given by element strides {batch, head}.
 *   hd in {16, 128}; every stride a multiple of 8 elements and every tensor base 16-byte aligned (anything else: VAA_E_UNSUPPORTED before any
 *   launch). NULL pointers, B < 0, H <= 0, Tmax <= 0 or a scale that is not finite and > 0: VAA_E_INVALID. B == 0: VAA_OK, nothing done.
 * Per (b, h): q and k_new are rotated at position pos[b] with vaa_model_rope's own arithmetic (same device function: the same bits, each
 *   rounded to bf16 once); the rotated k_new and v_new are stored into cache slot pos[b]; the query attends over keys 0 .. pos[b] inclusive
 *   (the new key straight from registers); the softmax runs in fp32 with the running max taken before the scaling; o is rounded to bf16 once.
 * Out-of-range rule: a row with pos[b] < 0 or pos[b] >= Tmax is skipped — its o is written as zeros, its cache is neither read nor written,
 *   and the device-failure word is raised (vaa_async_error() reports it; later library calls return VAA_E_LAUNCH until it is polled). No value
 *   of pos makes the kernel touch memory outside the views.
 * Determinism: no atomics and no hand-over between workgroups; the partial softmax states of a (b, h) pair are folded in a fixed order that
 *   depends on pos[b] alone, so the same arguments give the same bits and a row's result does not depend on the rest of the batch. */
int vaa_model_attention_decode(const uint16_t* q, const int64_t* q_str, const uint16_t* k_new, const int64_t* k_str, const uint16_t* v_new,
                               const int64_t* v_str, uint16_t* kcache, const int64_t* kc_str, uint16_t* vcache, const int64_t* vc_str,
                               const int32_t* pos, const float* cos_t, const float* sin_t, uint16_t* o, const int64_t* o_str, int B, int H,
                               int Tmax, int hd, float scale, void* stream);
/* ---- 4-bit block-quantised weights (inference only): the Llama projections of a model converted by quant.quantize_llm ----
 * THE FORMAT (this header defines it; it follows the layout of bitsandbytes' Linear4bit without double quantisation, but no copy of
 * bitsandbytes was available to compare a single value with):
 *   W        bf16 [N, K] row-major, K % 64 == 0 (anything else: VAA_E_UNSUPPORTED). A block is 64 consecutive elements of one row.
 *   absmax   float32 [N, K/64]: absmax[n, j] = max |W[n, 64 j .. 64 j + 63]| (exact: bf16 converts to fp32 exactly).
 *   table    16 float32 values, an ARGUMENT of every call (a HOST pointer, read before the call returns; nothing is compiled in).
 *   code     q[n, k] = the index i whose table[i] is nearest to the fp32 quotient W[n, k] / absmax[n, k / 64] (IEEE fp32 division, distances
 *            compared exactly); a tie goes to the smaller index; every element of a block whose absmax is 0 gets the smallest index i with
 *            table[i] == 0.
 *   codes    uint8 [N, K/2]: byte [n, i] = q[n, 2 i] << 4 | q[n, 2 i + 1] (the even element in the HIGH nibble).
 *   wq       the dequantised weight: wq[n, k] = bf16(table[q[n, k]] * absmax[n, k / 64]) — ONE fp32 product, rounded to bf16 once
 *            (round-to-nearest-even). Every consumer below sees exactly these wq, so a prefill through vaa_model_q4_dequant + a GEMM and a
 *            decode step through vaa_model_q4_gemv evaluate the same model.
 *   The quantiser itself is host-side (roboticattack_amd/quant.py: quantize_q4, on the CPU or the GPU with the same codes).
 * Both entry points: NULL pointers (res excepted), N < 1 or K < 64: VAA_E_INVALID; K % 64 != 0, or a device base address (codes, absmax, out /
 * x, res, y) that is not 16-byte aligned: VAA_E_UNSUPPORTED before any launch. */
/* out_bf16 [N, K] = wq. */
int vaa_model_q4_dequant(const uint8_t* codes, const float* absmax, const float* table, int N, int K, uint16_t* out_bf16, void* stream);
/* y[m, n] = bf16(res[m, n] + sum_k x[m, k] * wq[n, k]): x bf16 [M, K] contiguous, res (may be NULL) and y bf16 [M, N] contiguous; fp32
 * accumulation on the matrix cores, one rounding. 1 <= M <= 16 (M > 16: VAA_E_UNSUPPORTED — dequantise and run a GEMM; M < 0: VAA_E_INVALID;
 * M == 0: VAA_OK, nothing done). One launch; every code byte is read once.
 * Determinism: no atomics, no hand-over between workgroups, no waiting on memory another wave writes; the split over K inside a workgroup is
 * folded in a fixed order, so the same arguments give the same bits, and row m of y depends on row m of x (and res) alone. */
int vaa_model_q4_gemv(const uint16_t* x, int M, const uint8_t* codes, const float* absmax, const float* table, int N, int K,
                      const uint16_t* res, uint16_t* y, void* stream);
/* ---- 8-bit weights and activations with bf16 outlier columns (inference only): a model converted by quant.quantize_llm(model, "int8") ----
 * THE FORMAT AND THE ARITHMETIC (this header defines them; they follow LLM.int8 — Dettmers et al. 2022, what transformers' load_in_8bit gets
 * from bitsandbytes — vector-wise absmax scales, integer products, a threshold split — but bitsandbytes does not exist on this platform and not
 * one value was compared with it: this is this project's statement of the method). Every fp32 operation below is a separately rounded IEEE
 * operation (no fused multiply-add, correctly rounded division); rint is round-to-nearest-even.
 *   Weights W bf16 [N, K] row-major, K % 64 == 0, 64 <= K <= 133120 (127^2 K < 2^31: the int32 sum cannot overflow):
 *     wscale   float32 [N]: wscale[n] = max_k |W[n, k]| (exact).
 *     q        int8 [N, K] row-major: q[n, k] = clamp(rint(127 W[n, k] / wscale[n]), -127, 127), the product exact and the quotient formed in fp64
 *              (a quotient of two bf16 numbers that is not a half-integer is further than 2^-18 from one, so the fp64 rounding never makes a
 *              tie: this is rint of the exact quotient); a zero row has zero codes. The quantiser is host-side (quant.quantize_q8).
 *     wdq      the dequantised weight: wdq[n, k] = bf16((float(q[n, k]) * wscale[n]) / 127).
 *   Activations x bf16 [M, K], per call, threshold t >= 0 (fp32; t == 0: no outlier split):
 *     outlier  column k is an outlier when t > 0 and max_m |x[m, k]| >= t — the maximum over ALL M rows of the call: a row's result depends on
 *              the other rows of its call unless t == 0.
 *     ascale   float32 [M]: ascale[m] = max over the non-outlier k of |x[m, k]| (0 when every column is an outlier).
 *     xq       int8 [M, K]: 0 on outlier columns and in a row with ascale[m] == 0; elsewhere, with inv = 127 / ascale[m] (one division per
 *              row), xq[m, k] = clamp(rint(x[m, k] * inv), -127, 127).
 *     outliers int32 [K + 1] in caller-owned memory: outliers[0] = the count, outliers[1 .. count] = the outlier columns in ascending order;
 *              the rest of the K + 1 words is scratch and holds no defined value afterwards.
 *   Result, for every m < M, n < N:
 *     acc      = sum_k xq[m, k] q[n, k], exact in int32.
 *     o        = the sum over the outlier columns k, ascending, starting from 0, of x[m, k] * wdq[n, k]: o = o + (x * wdq).
 *     y[m, n]  = bf16((((float(acc) * (ascale[m] * wscale[n])) / 16129) + o) + res[m, n]); float(acc) rounds to nearest even; without res the
 *              last addition is not made.
 * Both entry points: M == 0: VAA_OK, nothing done. NULL pointers (res excepted), M < 0, N < 1, K < 64, a threshold that is negative or not
 * finite: VAA_E_INVALID; K % 64 != 0, K > 133120, or a base address of x, xq, q, res, y that is not 16-byte aligned (ascale, wscale, outliers:
 * 4-byte): VAA_E_UNSUPPORTED before any launch. Nothing outside xq, ascale, the K + 1 words of outliers and y is written. No atomics, no
 * hand-over between workgroups: the same arguments give the same bits. */
/* x -> xq, ascale, outliers. Any M >= 1. M <= 16: one launch (every workgroup owns one row and forms the column maxima of all M rows itself);
 * more rows: three launches on the stream (column flags, the rows, the ordered list). */
int vaa_model_q8_act_quant(const uint16_t* x, int M, int K, float threshold, int8_t* xq, float* ascale, int32_t* outliers, void* stream);
/* y from what vaa_model_q8_act_quant wrote (x is read on the outlier columns only). form 0: M <= 16 runs the split-K form (one launch, every
 * weight byte read once by one lane of one workgroup), more rows the tiled integer GEMM (a workgroup owns 128 rows n x 64 rows m: the weights
 * are read ceil(M / 64) times). form 1 forces the split-K form (M > 16: VAA_E_UNSUPPORTED), form 2 the GEMM; any other form: VAA_E_INVALID.
 * Both forms end in the same device function, so they give the same bits for the same call. */
int vaa_model_q8_matmul(const int8_t* xq, const float* ascale, const int32_t* outliers, const uint16_t* x, int M, const int8_t* q,
                        const float* wscale, int N, int K, const uint16_t* res, uint16_t* y, int form, void* stream);
#ifdef __cplusplus
}
#endif
#endif
