/*
 * vaa.h — C-ABI of libvaa_hip.so: the MI355X (gfx950) replacement for the UADA/UPA/TMA inner attack loop's
 * patch operators of William-wAng618/roboticAttack.
 *
 * The reference is pure Python and has no FFI; the seams this library replaces are the Python operator calls
 * listed per entry point below (file:line under the reference tree). INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add to call them.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only. Every pointer marked `dev` is a DEVICE pointer owned by the
 *     caller (e.g. a PyTorch-ROCm tensor's data_ptr()); `host` pointers are ordinary host memory read during
 *     the call. Nothing is allocated or freed by the library; scratch comes from the caller via *_ws_bytes().
 *   - Every function returns VAA_OK (0) or a negative VAA_E_* code; vaa_last_error() returns a thread-local
 *     message for the last failure on the calling thread.
 *   - Kernels are enqueued on the caller's `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and the call returns without synchronising. Re-entrant per stream; no global mutable state.
 *   - Images are 224x224 (the reference hard-codes this size: UADA.py:60, modeling_prismatic.py:120).
 */
#ifndef VAA_H_
#define VAA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAA_OK 0
#define VAA_E_INVALID (-1)     /* bad argument (null pointer, size out of range, unknown mode) */
#define VAA_E_UNSUPPORTED (-2) /* valid request the kernels do not cover (e.g. patch larger than 224) */
#define VAA_E_LAUNCH (-3)      /* HIP runtime reported an error at launch */
#define VAA_E_WORKSPACE (-4)   /* workspace missing or too small */
#define VAA_E_NODEVICE (-5)    /* no gfx950 device visible */

#define VAA_IMG 224

/* paste-mask rule */
#define VAA_MASK_LT_M20 0 /* keep patch where !(canvas < -20)  : apply_random_patch_batch, appply_random_transform.py:131 */
#define VAA_MASK_NE_M100 1 /* keep patch where canvas != -100   : paste_patch_fix / random_paste_patch, :153 :179; geometry=0 only
                              (with a warp the rule would hinge on the rounding of -100*(sum of weights): VAA_E_UNSUPPORTED) */

/* loss modes (K3) */
#define VAA_LOSS_UADA 0     /* w^2*mean((r-t)^2) + 1/CE                       UADA.py:145-148,381-406 */
#define VAA_LOSS_UADA_DDP 1 /* w^2*mean((r-t)^2)                              UADA_ddp.py:99-124,203-206 */
#define VAA_LOSS_UPA 2      /* alpha*mean(cos+1) + beta/(mean||e-l|| + 1e-3)  UPA.py:367-387 */
#define VAA_LOSS_CE 3       /* scale*CE (TMA target CE, UPA guide / -CE)      TMA.py:148, UPA.py:143-150 */

/* logits element type */
#define VAA_DTYPE_F32 0
#define VAA_DTYPE_BF16 1

/* logits layout */
#define VAA_LAYOUT_FULL 0 /* [B,S,V], S = 256 + L: row (b, S-L+k) predicts labels[b,k+1] (HF shift; UADA.py:385) */
#define VAA_LAYOUT_ROWS 1 /* [R,V]: only the labelled rows, in (b,k) row-major order of labels[b,k+1] != -100 */

/* gradient storage of vaa_loss_rows_fwd_bwd */
#define VAA_GRAD_FULL 0  /* [R,V], the logits' dtype */
#define VAA_GRAD_SLICE 1 /* [R,256]: the action columns 31744..31999 only (UADA_DDP / UPA: the gradient is zero elsewhere) */
#define VAA_SEG_UPA_MAX_GROUPS 32 /* groups of one vaa_loss_rows_fwd_bwd_seg_upa call: their parameters travel in the launch's arguments */

/* optimiser modes (K4) */
#define VAA_OPT_ADAMW_HF 0 /* transformers==4.40.1 AdamW.step (eps outside bias correction) + clamp(0,1)  UADA.py:155-156 */
#define VAA_OPT_PGD_SIGN 1 /* p = clamp(p - lr*sign(g), 0, 1)                                            TMA.py:171-175 */

const char* vaa_last_error(void);
int vaa_version(void);
/*
 * PROCESS-WIDE STATE — the two places where this library is NOT the stateless, per-stream re-entrant operator set SURVEY.md section 8b sketched
 * (everything else is: caller-owned memory and streams, no allocation, no synchronisation, thread-local error text):
 *   (1) the device-failure word behind vaa_async_error() below: one pinned host word per process, STICKY, not attributed to a stream;
 *   (2) the per-dispatch profiler vaa_prof_*: one record table per process behind a mutex.
 * Also per process, but invisible to callers: a launch-tag counter and "one stream at a time has a waiting grid in flight" bookkeeping for the
 * launches whose workgroups wait for each other (vaa_head_slice_fwd_bwd; the opt-in one-launch form of vaa_loss_rows_fwd_bwd) — they only decide
 * between the one-launch and the two-launch form of those calls, never their results.
 *
 * Device-side failures surface here and NEVER as a silent NaN: a kernel that has to give up (vaa_head_slice_fwd_bwd's one-launch form and the opt-in
 * one-launch K3, when a hand-over runs out of polls) NaN-poisons its outputs AND sets a bit in a pinned host word. The word is process-wide and STICKY:
 * from then on EVERY library call on any stream or thread returns VAA_E_LAUNCH (reason in vaa_last_error()) — the failure is not attributed
 * to a stream, and no call consumes it — until vaa_async_error() is called: the explicit poll reports the failure (VAA_E_LAUNCH) and clears
 * the word. The attack loops poll it behind their once-per-outer-iteration read-back, before anything is written to disk (UADA.py:257-275).
 * Returns VAA_OK or VAA_E_LAUNCH.
 */
int vaa_async_error(void);
/* VAA_OK when a gfx950 device is visible to the HIP runtime, else VAA_E_NODEVICE. */
int vaa_device_check(void);

/*
 * Per-dispatch timing of the library's own kernels (measurement aid; no reference counterpart). While armed, every kernel the library
 * launches is dispatched with its own start/stop event pair bound to THAT dispatch (hipExtLaunchKernel): its elapsed time is the
 * dispatch's begin-to-end GPU time, the quantity `rocprofv3 --kernel-trace` reports, read inside a running step without marker packets.
 *   vaa_prof_start(capacity): allocate (once) `capacity` event pairs, drop earlier records, arm; capacity 0 disarms. Dispatches beyond
 *             the capacity run unprofiled. Do not arm during stream capture.
 *   vaa_prof_stop(): disarm; returns the number of records.
 *   vaa_prof_get(i, &name, &usec): waits for record i's dispatch and returns the kernel's name (static string) and duration in us.
 * Process-wide state behind a mutex; the launching thread arms / disarms between steps.
 */
int vaa_prof_start(int capacity);
int vaa_prof_stop(void);
int vaa_prof_get(int i, const char** name, float* usec);

/*
 * K1 — replaces RandomPatchTransform.apply_random_patch_batch (appply_random_transform.py:104-136) followed by the
 * caller's `.to(torch.bfloat16)` (UADA.py:142), and paste_patch_fix (:160-188) with mask_mode=VAA_MASK_NE_M100,
 * geometry=0. The random draws (:120-128) stay on the host so the RNG streams match; their results come in as xy/theta.
 *   img_u8   dev  [B,224,224,3] uint8 HWC (what PIL/ToTensor sees, :108)
 *   patch    dev  [3,ph,pw] float32
 *   xy       dev  [B,2] int32 (x,y) paste position (:123-125)
 *   theta    dev  [B,6] float32 row-major 2x3 affine (rows 0-1 of combined_transform_matrix(), :88-96); ignored if !geometry
 *   mean6/std6 host [6] float32: channels 0-2 -> first normalisation, 3-5 -> second (UADA.py:56-57)
 *   out_bf16 dev  [B,6,224,224] bfloat16 bits: the model's pixel_values
 *   keep_bits dev [B,3,224*224/8] uint8 or NULL: bit (p&7) of byte p>>3 is 1 where channel c of pixel p=i*224+j
 *             shows the patch (the `torch.where` mask, :131); consumed by vaa_patch_grad_gather
 */
int vaa_patch_apply_fwd(const uint8_t* img_u8, const float* patch, const int32_t* xy, const float* theta, int B, int ph,
                        int pw, int geometry, int mask_mode, const float* mean6, const float* std6, uint16_t* out_bf16,
                        uint8_t* keep_bits, void* stream);

/*
 * K1 in TILE-MAJOR form — the same values as vaa_patch_apply_fwd, laid out as the operands of the two ViT patch-embed GEMMs
 * (modeling_prismatic.py:120-123 -> timm PatchEmbed, Conv2d(3, D, 14, stride 14) == a GEMM over 588-pixel tiles), for callers that own the
 * patch-embed weights (K2' below): the [B,6,224,224] tensor and its two 19 MB im2col copies per step are never made.
 *   pdesc     dev [B,4] or NULL: per-image patches as in vaa_patch_apply_fwd_multi (ph/pw are then upper bounds)
 *   out0,out1 dev bf16 [B,256,588]: tile t = ty*16 + tx, element c*196 + y*14 + x; out0 = first normalisation (channels 0-2 of
 *             pixel_values), out1 = second (channels 3-5). e_k = out_k @ W_k^T + b_k with W_k = conv weight [D,3,14,14] flattened to [D,588]
 *   keep_tiles dev u16 [B,3,256,14] or NULL: bit x of word (c, t, y) = channel c of pixel (14 ty + y, 14 tx + x) shows the patch
 *   tile_flags dev u32 [B,256] or NULL: != 0 when tile t holds a kept pixel in any channel (the tile list K2' evaluates)
 */
int vaa_patch_apply_fwd_tiles(const uint8_t* img_u8, const float* patch, const int32_t* pdesc, const int32_t* xy, const float* theta, int B,
                              int ph, int pw, int geometry, int mask_mode, const float* mean6, const float* std6, uint16_t* out0,
                              uint16_t* out1, uint16_t* keep_tiles, uint32_t* tile_flags, void* stream);

/*
 * K2 — replaces the autograd backward of K1 to the patch (implicit in `.backward()`, UADA.py:148): bf16->f32 cast,
 * /std of both normalisations summed, where-mask, grid_sample-backward scatter, slice, sum over the batch.
 *   gout_bf16 dev [B,6,224,224] bfloat16 bits: dL/d pixel_values from the model
 *   patch, xy, theta, geometry, mask_mode: as given to K1 for the same step
 *   keep_bits dev: K1's mask output, or NULL to recompute the mask from `patch`
 *   std6     host [6]
 *   gpatch   dev  [3,ph,pw] float32, overwritten with dL/d patch (sum over the B images); NULL leaves the final fixed-order sum to
 *             vaa_step_epilogue[_update]: the vaa_patch_grad_partials(B) partial tiles [parts][3*ph*pw] f32 then sit at the start of ws
 *   ws       dev  scratch of at least vaa_patch_grad_ws_bytes(B,ph,pw) bytes (contents undefined on entry and exit)
 * Numerics: every bilinear contribution fl(G*w) is accumulated as an integer (quantum 2^-30 of the largest |G| a workgroup meets), the
 * partial tiles are added in a fixed order: the same arguments give the same bits, for every patch size up to 224x224 (no global or
 * floating-point atomics); the result is the exact sum of the reference's fp32 products rounded once. A non-finite upstream value makes
 * (at least) the patch rows it touches NaN.
 */
size_t vaa_patch_grad_ws_bytes(int B, int ph, int pw);
int vaa_patch_grad_gather(const uint16_t* gout_bf16, const float* patch, const int32_t* xy, const float* theta,
                          const uint8_t* keep_bits, int B, int ph, int pw, int geometry, int mask_mode, const float* std6,
                          float* gpatch, void* ws, size_t ws_bytes, void* stream);

/*
 * resize_patch=True (BASELINE config 5) — replaces, for the whole batch at once, `patch = transforms.Resize((height, width))(patch)`
 * with `scale = random.uniform(0.61, 1.39)` (appply_random_transform.py:113-116; semantics of SURVEY.md Appendix A-D2: every image
 * scales the BASE patch), the paste/warp of every image's own resized patch (:118-136) and their autograd backward.
 * The draws stay on the host; their results travel as a per-image descriptor:
 *   pdesc    dev  [B,4] int32 = {h_b, w_b, offset_b, 0}: image b's patch is [3,h_b,w_b] float32 at packed + offset_b
 *             (offsets in floats; regions must not overlap; vaa_patch_*_multi read sizes from here, max_h/max_w bound them)
 * vaa_patch_resize_fwd: packed[offset_b ...] = antialiased bilinear resize of patch [3,ph,pw] to (h_b, w_b) — torchvision Resize on a
 *             tensor == torch F.interpolate(mode='bilinear', antialias=True, align_corners=False); bit-exact against torch's CPU kernel.
 * vaa_patch_resize_bwd: gpatch [3,ph,pw] = sum_b adjoint(resize_b)(gpacked_b), overwritten; ws >= vaa_patch_resize_ws_bytes(B,ph,pw)
 *             (one partial per image group — one image per group until the batch alone fills the chip; 0 for a single group).
 * vaa_patch_apply_fwd_multi / vaa_patch_grad_gather_multi: K1 / K2 with per-image patches. K2's output gpacked has the layout of
 *             packed and holds d L / d (every image's own resized patch); elements between the patches are not written.
 * Launch counts do not depend on B: forward = resize + K1, backward = K2 + resize adjoint + fixed-order sum over the images.
 */
int vaa_patch_resize_fwd(const float* patch, int ph, int pw, const int32_t* pdesc, int B, float* packed, void* stream);
size_t vaa_patch_resize_ws_bytes(int B, int ph, int pw);
int vaa_patch_resize_bwd(const float* gpacked, int ph, int pw, const int32_t* pdesc, int B, float* gpatch, void* ws, size_t ws_bytes,
                         void* stream);
int vaa_patch_apply_fwd_multi(const uint8_t* img_u8, const float* packed, const int32_t* pdesc, const int32_t* xy, const float* theta,
                              int B, int max_h, int max_w, int geometry, int mask_mode, const float* mean6, const float* std6,
                              uint16_t* out_bf16, uint8_t* keep_bits, void* stream);
int vaa_patch_grad_gather_multi(const uint16_t* gout_bf16, const float* packed, const int32_t* pdesc, const int32_t* xy,
                                const float* theta, const uint8_t* keep_bits, int B, int max_h, int max_w, int geometry, int mask_mode,
                                const float* std6, float* gpacked, void* stream);

/*
 * colorjitter (K0c) — a per-image photometric draw on the BASE patch in front of the same per-image-patch kernels, and its adjoint. The
 * reference carries a `colorjitter=` flag from TMA.py into apply_random_patch_batch and never acts on it, so the
 * arithmetic is defined HERE. With p = patch [3,ph,pw] in [0,1], N = ph*pw, gray(y) = 0.299 y_R + 0.587 y_G + 0.114 y_B and image b's
 * factors (beta, kappa, sigma) = factors[b] (brightness, contrast, saturation; no hue term), in fp32 with every a*x + c one FMA on a rounded c:
 *     y1 = clamp(beta*p, 0, 1)
 *     m  = (1/N) * sum over the texels of gray(y1)                (one scalar per image; fixed-order fp64 sum, rounded once)
 *     y2 = clamp(kappa*y1 + (1-kappa)*m, 0, 1)
 *     y3 = clamp(sigma*y2 + (1-sigma)*gray(y2), 0, 1)             (gray per texel)
 * factors (1, 1, 1) return p bit for bit. The draws stay on the host (RandomPatchTransform: 3*B random.uniform calls behind the placement draws).
 *   factors  dev  [B,3] float32
 *   pdesc    dev  [B,4] int32 = {ph, pw, offset_b, 0} as above — every image's patch has the base patch's size; an entry of another size
 *             leaves that image unwritten (its adjoint zero) and raises the device-failure word (vaa_async_error)
 * Forward, one launch: packed[offset_b ...] = y3 of image b — the layout the per-image-patch forms of K1 / K2 / K2' read.
 * Adjoint: gpatch [3,ph,pw] = sum_b adjoint_b(gpacked_b), overwritten — the exact derivative of the above with torch.clamp's gate (the gradient
 *             passes where 0 <= pre-clamp <= 1, bounds included), recomputed from patch and factors (no forward state), including both
 *             coupling terms: the per-texel gray term of the saturation stage and the whole-patch mean term of the contrast stage,
 *             (1-kappa)/N * w_c * (sum over texels and channels of the gated gradient G2' in front of the contrast clamp).
 *             ws >= the adjoint's workspace size for (B,ph,pw): one partial per image, 0 for B = 1. Two launches whatever B is (per-image adjoint,
 *             fixed-order fp64 sum over the images); the same arguments give the same bits.
 */
int vaa_patch_jitter_fwd(const float* patch, int ph, int pw, const float* factors, const int32_t* pdesc, int B, float* packed, void* stream);
size_t vaa_patch_jitter_ws_bytes(int B, int ph, int pw);
int vaa_patch_jitter_bwd(const float* gpacked, const float* patch, int ph, int pw, const float* factors, const int32_t* pdesc, int B,
                         float* gpatch, void* ws, size_t ws_bytes, void* stream);

/*
 * K6 — smoothness and printability terms of the patch: total variation (TV) and the non-printability score (NPS), values and gradient in ONE
 * launch. The reference has no such term (they come with Thys et al.'s adversarial-patch code and Sharif et al.'s NPS), so the arithmetic is
 * defined HERE. With p = patch [3,ph,pw], N = ph*pw texels t = (i,j), N3 = 3*N, q = palette [K,3] (1 <= K <= 64) and eps = 1e-6:
 *     TV(p)  = ( sum_c sum_i sum_{j<pw-1} |p[c,i,j+1] - p[c,i,j]|  +  sum_c sum_{i<ph-1} sum_j |p[c,i+1,j] - p[c,i,j]| ) / N3
 *     d_k(t) = sqrt( sum_c (p[c,t] - q[k,c])^2 + eps )
 *     NPS(p) = ( sum_t min_k d_k(t) ) / N3
 *     dTV/dp[c,i,j]  = ( sgn(p - left) - sgn(right - p) + sgn(p - up) - sgn(down - p) ) / N3     (absent neighbours contribute nothing; sgn(0) = 0)
 *     dNPS/dp[c,t]   = (p[c,t] - q[k*,c]) / d_k*(t) / N3,   k* = the lowest index attaining the fp32 minimum
 * The regulariser w_tv*TV + w_nps*NPS is minimised (as every attack loss is). Rounding sequence, fp32, every FMA explicit:
 *     e_c = p[c,t] - q[k,c];   d_k = sqrt( fma(e_2, e_2, fma(e_1, e_1, e_0*e_0)) + eps )  (correctly rounded sqrt);   k* by `d < best`, k ascending
 *     s_c = ((sgn(p - left) - sgn(right - p)) + sgn(p - up)) - sgn(down - p)            (differences rounded once; the sum is a small integer)
 *     c_tv = (float)((double)w_tv / N3),  c_nps = (float)((double)w_nps / N3)
 *     r_c = fma(c_tv, s_c, c_nps * (e_c / d_k*))        both weights non-zero
 *         = c_nps * (e_c / d_k*)                        w_tv == 0 (the TV gradient work is skipped)
 *         = c_tv * s_c                                  w_nps == 0
 * NaN rule: a NaN texel gives a NaN distance to every colour; a NaN distance is taken by the minimum and kept, so that texel's three gradient
 * elements and the NPS sum are NaN (sgn(NaN) = 0, torch's rule: the TV gradient of its neighbours stays finite).
 *   patch    dev  [3,ph,pw] float32
 *   palette  dev  [K,3] float32, or NULL with K = 0 when w_nps == 0 (the NPS value is then 0)
 *   grad     dev  [3,ph,pw] float32 or NULL (values only): accumulate = 0 writes r, accumulate = 1 writes grad + r — ONE rounded add of exactly
 *             the r the write form produces
 *   part     dev  float64 [vaa_patch_reg_parts(ph,pw)][2] out: per workgroup (256 consecutive texels) {sum of the right / down |differences|
 *             its texels own, sum of their min distances}, un-normalised, accumulated in a fixed order (the thread's own terms in channel order,
 *             a butterfly over the wave, the waves in order): the same arguments give the same bits. TV = sum(part[:,0]) / N3 and
 *             NPS = sum(part[:,1]) / N3 are folded by the caller when it wants them; the launch has no atomics and no hand-over.
 * VAA_E_INVALID before any launch: NULL patch or part, a non-finite weight, K > 64, K < 1 (or a NULL palette) while w_nps != 0.
 */
size_t vaa_patch_reg_parts(int ph, int pw);
int vaa_patch_reg(const float* patch, int ph, int pw, const float* palette, int K, float w_tv, float w_nps, float* grad, int accumulate,
                  double* part, void* stream);

/*
 * K3 — replaces HF Llama's `.loss` (via modeling_prismatic.py:404-415) + OpenVLAAttacker.weighted_loss
 * (UADA.py:381-406, UADA_ddp.py:99-124, UPA.py:367-387) and their autograd backward to the logits.
 *   logits   dev  f32|bf16, layout FULL [B,S,V] or ROWS [R,V]. For ROWS pass S = R (the number of rows, which must equal the number
 *             of labelled positions): the call then builds the row map in `ws` and runs vaa_loss_rows_fwd_bwd (below); S = 0 (unknown)
 *             keeps the label-driven schedule
 *   labels   dev  [B,L] int64, already masked by the caller (mask_labels, UADA.py:371-379)
 *   params   host [4] float32: {w (MSE weight: 5 or --MSE_weights), alpha, beta, scale (1/accumulate_steps)}
 *   scalars  dev  [8] float32 out: {total, CE, w^2*MSE, aux0 (UPA angle), aux1 (UPA dist), #CE rows, #action rows, UAD}
 *   pred_tokens dev [B*(L-1)] int32 or NULL: argmax action token (31744 + argmax of the 256-slice, UADA.py:395) per
 *             labelled row in (b,k) order (rows whose label is <= 2 get -1)
 *   glogits  dev or NULL: d total / d logits in the logits' dtype and layout. FULL: only labelled rows are written
 *             (zero the buffer once; rows never change while labels keep their shape). ROWS: every row is written.
 *   ws       dev scratch >= vaa_loss_ws_bytes(B,L)
 */
size_t vaa_loss_ws_bytes(int B, int L);
int vaa_loss_fwd_bwd(const void* logits, int dtype, int layout, const int64_t* labels, int B, int S, int L, int V, int mode,
                     const float* params, float* scalars, int32_t* pred_tokens, void* glogits, void* ws, size_t ws_bytes,
                     void* stream);
/* The same with one more output: pred_full_tokens dev [B*(L-1)] or NULL = argmax over ALL V logits of every labelled row
 * (`action_logits.argmax(dim=2)`, UADA.py:165-167, TMA.py:148-149: what the reference's relative-distance / L1 / ASR metrics and the
 * best-patch selection read), -1 on unlabelled positions. pred_tokens stays the action-slice argmax that feeds UAD (UADA.py:395). */
int vaa_loss_fwd_bwd_ex(const void* logits, int dtype, int layout, const int64_t* labels, int B, int S, int L, int V, int mode,
                        const float* params, float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens, void* glogits, void* ws,
                        size_t ws_bytes, void* stream);

/*
 * K3 on the labelled rows with a prebuilt row map (LM head + loss on labelled rows only) — what the attack
 * loops use: labels are fixed during the innerLoop steps of an outer iteration (UADA.py:130-133), so the map is built once per outer
 * iteration and a step never touches the label matrix.
 *   vaa_loss_rowmap_build: rowmap dev (>= vaa_loss_rowmap_bytes(B,L)) = int32 {R, #action rows, 0, 0} followed by {b, k, label, ord}
 *             per labelled position in (b,k) row-major order of labels[b,k+1] != -100 (the order of VAA_LAYOUT_ROWS).
 *   vaa_loss_rows_fwd_bwd: logits dev [R,V] f32|bf16 in that order; R (host) must equal the map's count (else scalars[0] = NaN).
 *             pred_tokens      dev [B*(L-1)] or NULL: 31744 + argmax of the 256 action logits (UADA.py:395, feeds UAD); -1 elsewhere
 *             pred_full_tokens dev [B*(L-1)] or NULL: argmax over ALL V logits (`action_logits.argmax(dim=2)`, UADA.py:165-167,
 *                              TMA.py:148-149: relative distance, L1 / ASR metrics, best-patch selection); -1 on unlabelled positions
 *             grad dev or NULL, grad_kind VAA_GRAD_FULL [R,V] | VAA_GRAD_SLICE [R,256] (only for UADA_DDP / UPA, whose gradient is
 *                              confined to the action columns: the LM-head backward then contracts over 256 columns, not 32,064)
 *             ws >= vaa_loss_rows_ws_bytes(R). Rows are split over 2-4 workgroups so that 128 rows fill the 256 CUs; in UADA_DDP
 *             mode the gradient is written by the same pass that reads the logits. Full-row gradients whose scale needs the folded
 *             scalars (UADA's 1/CE^2 term, UADA.py:145-148; CE, TMA.py:148) can be ONE launch too — statistics, grid-wide hand-over,
 *             gradient from the registers, every row read once — ONLY with VAA_K3_ONE_PASS=1 in the environment (opt-in since
 *             round 4: 2.8 us per call against a residency assumption no launch API guarantees) and when the grid takes at most half
 *             of the device's resident slots, the stream is not being captured and no other stream of the process has such a launch
 *             in flight; else two launches with the same bits in every output. A hand-over that times out NaN-poisons the gradient AND
 *             raises vaa_async_error() (every later library call fails with VAA_E_LAUNCH until the word is polled).
 */
size_t vaa_loss_rowmap_bytes(int B, int L);
int vaa_loss_rowmap_build(const int64_t* labels, int B, int L, void* rowmap, size_t rowmap_bytes, void* stream);
size_t vaa_loss_rows_ws_bytes(int R);
int vaa_loss_rows_fwd_bwd(const void* logits, int dtype, const void* rowmap, int R, int B, int L, int V, int mode, const float* params,
                          float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens, void* grad, int grad_kind, void* ws,
                          size_t ws_bytes, void* stream);

/*
 * Split form of vaa_loss_rows_fwd_bwd for the data-parallel step (UADA_ddp.py:199-209), whose backward does not wait for the loss scalars:
 *   vaa_loss_rows_stats : the statistics pass alone; in VAA_LOSS_UADA_DDP mode it also writes the gradient (grad may be NULL; other modes
 *             need the folded scalars for their gradient and must use vaa_loss_rows_fwd_bwd). ws as in vaa_loss_rows_fwd_bwd.
 *   vaa_step_epilogue   : ONE launch between the backward and the gradient exchange — replaces K2's final reduce launch, K3's finishing
 *             launch and the packing of the DDP message (dist.PatchGradSync):
 *               msg[0..n)    = sum of K2's `nparts` partial tiles [nparts][n] (n = 3*ph*pw), the fixed order of
 *                              vaa_patch_grad_gather: bitwise the gradient that call would have written
 *               rowmap != NULL: the statistics in loss_ws (left by vaa_loss_rows_stats with the same R, B, L, V, mode, params) are folded:
 *                              scalars[8], pred_tokens, pred_full_tokens as vaa_loss_rows_fwd_bwd writes them
 *               rowmap == NULL: scalars is an INPUT (already final)
 *               msg[n..n+4)  = {CE, w^2*MSE, UAD, total}: the logging scalars that travel with the gradient (C3 + C4 in one all-reduce)
 */
int vaa_loss_rows_stats(const void* logits, int dtype, const void* rowmap, int R, int B, int L, int V, int mode, const float* params, void* grad,
                        int grad_kind, void* ws, size_t ws_bytes, void* stream);
int vaa_step_epilogue(const float* partials, int nparts, int n, const void* rowmap, int R, int B, int L, int V, int mode,
                      const float* params, const void* loss_ws, size_t loss_ws_bytes, float* scalars, int32_t* pred_tokens,
                      int32_t* pred_full_tokens, float* msg, void* stream);
/* Single-GPU form (UADA.py:148-157: nothing sits between the gradient and optimizer.step()): the epilogue also applies K4 — vaa_patch_update
 * with grad_scale = 1 and no L1 clip — to every gradient element as it is produced (same per-element arithmetic: patch / m / v get the
 * bits the separate launch would write). stat_part dev f64 [ceil(n/64)][2] or NULL: per-block {sum |g|, sum g}; their sums give K4's
 * logged {sum|g|, mean g = sum g / n}. */
int vaa_step_epilogue_update(const float* partials, int nparts, int n, const void* rowmap, int R, int B, int L, int V, int mode,
                             const float* params, const void* loss_ws, size_t loss_ws_bytes, float* scalars, int32_t* pred_tokens,
                             int32_t* pred_full_tokens, float* msg, float* patch, float* m, float* v, int opt_mode, float lr, float beta1,
                             float beta2, float eps, int step, double* stat_part, void* stream);

/*
 * maskidx SWEEP — P patch groups optimised in ONE step (BASELINE config 5's maskidx families, the released UADA-dof1 / UADA-dof1~3 pairs): the
 * batch is P groups of Bp consecutive images, group p with its own labels (its own maskidx) and its own patch; every group sees the same frames
 * and transform draws. Group p's outputs are those of a standalone step on its Bp images alone.
 *   vaa_loss_rowmap_build_seg: rowmap dev (>= vaa_loss_rowmap_seg_bytes(B,L,P)) = the ordinary map of all B = P*Bp label rows (header
 *             {R, #action rows, P, Bp}; the rows exactly vaa_loss_rowmap_build's), a table {first row, rows, action rows, 0} per group and every
 *             group's own ordinary map (vaa_loss_rowmap_build on its Bp rows). vaa_head_slice_fwd_bwd (K3s) and vaa_head_loss_rows_stats (K3h) accept
 *             it in VAA_LOSS_UADA_DDP mode: each row's gradient is normalised by ITS GROUP's action-row count, so dhidden / grad_slice / the row
 *             statistics of group p's rows are bit for bit those of the call on group p's rows alone with the group's ordinary map (an ordinary map
 *             gives the old bits). Folds inside those calls (scalars != NULL, vaa_head_loss_rows_finish) treat the map as ONE batch: per-group
 *             scalars come from vaa_step_epilogue_seg. UPA's batch means are not per group: the segmented map serves VAA_LOSS_UADA_DDP there,
 *             VAA_LOSS_CE through vaa_loss_rows_fwd_bwd_seg (the target sweep below) and VAA_LOSS_UPA — whose batch means ARE folded per group —
 *             through vaa_loss_rows_fwd_bwd_seg_upa (the UPA sweep below).
 *   vaa_step_epilogue_seg: ONE launch, vaa_step_epilogue per group (the same kernel: vaa_step_epilogue is its one-group case): partials
 *             [P*nparts][n] (group p's nparts tiles at p*nparts: K2' with one partial per image, nparts = Bp) ->
 *               msg[p*n .. (p+1)*n)  = group p's fixed-order sum: bitwise vaa_step_epilogue over those nparts tiles
 *               rowmap (segmented, or an ordinary map with P = 1) != NULL: group p folded with its own map into scalars[8p .. 8p+8) and rows
 *                                    p*Bp .. of pred_tokens / pred_full_tokens [B, L-1] (VAA_LOSS_UADA_DDP; loss_ws as the K3s / K3h call left it)
 *               msg[P*n + 4p ..)     = group p's {CE, w^2*MSE, UAD, total}; rowmap == NULL (pass-through): ZEROS — a SUM all-reduce of the tail
 *                                    can never grow stale values by world^steps
 *   vaa_step_epilogue_seg_update: the same + K4 (HF-AdamW | PGD + clamp, shared lr / step) on every element of patch / m / v [P*n] as it is
 *             produced (vaa_step_epilogue_update's arithmetic); stat_part dev f64 [P][ceil(n/64)][2] or NULL: group p's per-block {sum |g|, sum g},
 *             bitwise the stat_part a standalone vaa_step_epilogue_update writes (their sums give the group's logged K4 stats).
 *   vaa_patch_update_seg: vaa_patch_update on each of P groups of n elements (patch, g, m, v [P*n]) in one launch — every group its own L1 clip
 *             and statistics, stats dev [P,2] f32 or NULL: bit for bit P separate vaa_patch_update calls (the data-parallel sweep after its all-reduce;
 *             the same kernel: vaa_patch_update is its one-group case).
 */
size_t vaa_loss_rowmap_seg_bytes(int B, int L, int P);
int vaa_loss_rowmap_build_seg(const int64_t* labels, int B, int L, int P, void* rowmap, size_t rowmap_bytes, void* stream);
int vaa_step_epilogue_seg(const float* partials, int nparts, int n, int P, const void* rowmap, int R, int B, int L, int V, int mode,
                          const float* params, const void* loss_ws, size_t loss_ws_bytes, float* scalars, int32_t* pred_tokens,
                          int32_t* pred_full_tokens, float* msg, void* stream);
int vaa_step_epilogue_seg_update(const float* partials, int nparts, int n, int P, const void* rowmap, int R, int B, int L, int V, int mode,
                                 const float* params, const void* loss_ws, size_t loss_ws_bytes, float* scalars, int32_t* pred_tokens,
                                 int32_t* pred_full_tokens, float* msg, float* patch, float* m, float* v, int opt_mode, float lr, float beta1,
                                 float beta2, float eps, int step, double* stat_part, void* stream);
int vaa_patch_update_seg(float* patch, const float* g, float* m, float* v, int n, int P, int mode, float lr, float beta1, float beta2,
                         float eps, int step, float l1_clip, float grad_scale, float* stats, void* stream);

/*
 * TARGET SWEEP — P TMA patch groups (TMA.py's target-token CE, one (maskidx, target action) pair per group: the released T-dof1 .. T-dof7 family)
 * in ONE step. The gradient of the cross-entropy needs every logit, so the head stays the hipBLASLt GEMM — run ONCE over the rows of all groups —
 * and K3 takes the segmented row map in VAA_LOSS_CE mode:
 *   vaa_loss_rows_fwd_bwd_seg: vaa_loss_rows_fwd_bwd (its two launches, the same kernels: that call is their one-batch case) on logits [R,V] of
 *             P groups of B/P images; rowmap from vaa_loss_rowmap_build_seg (groups may label different numbers of rows), or an ordinary map
 *             with P = 1 (the bits of vaa_loss_rows_fwd_bwd). Row r's gradient = scale / nrow_g (softmax - onehot) with nrow_g the row count of
 *             ITS group; one fold workgroup per group, past the gradient workgroups (no gradient waits for a fold), folds the group with its own
 *             map into scalars[8g .. 8g+8) and rows g*B/P .. of pred_tokens / pred_full_tokens [B, L-1]. At V = 32,064 a row is split into 4 parts
 *             for every R, so group g's gradient rows, scalars and prediction-map rows are bit for bit those of vaa_loss_rows_fwd_bwd on the
 *             group's logits rows alone with its ordinary map. VAA_LOSS_CE with VAA_GRAD_FULL only (else VAA_E_UNSUPPORTED); grad may be NULL
 *             (evaluation); always two launches (VAA_K3_ONE_PASS does not apply). scalars dev f32 [P,8]; the other arguments as
 *             vaa_loss_rows_fwd_bwd.
 *   vaa_step_epilogue_seg_tail[_update]: vaa_step_epilogue_seg[_update] in its pass-through form (K2's fixed-order sums of P groups, + K4) whose
 *             message tail carries scalars that are final already: msg[P*n + 4g ..) = scalars_in[8g + {1, 2, 7, 0}] = group g's {CE, w^2*MSE, UAD,
 *             total}. For the step whose scalars the loop reads; every other step keeps vaa_step_epilogue_seg's zero tail.
 */
int vaa_loss_rows_fwd_bwd_seg(const void* logits, int dtype, const void* rowmap, int R, int B, int L, int V, int P, int mode, const float* params,
                              float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens, void* grad, int grad_kind, void* ws,
                              size_t ws_bytes, void* stream);
int vaa_step_epilogue_seg_tail(const float* partials, int nparts, int n, int P, const float* scalars_in, float* msg, void* stream);
int vaa_step_epilogue_seg_tail_update(const float* partials, int nparts, int n, int P, const float* scalars_in, float* msg, float* patch, float* m,
                                      float* v, int opt_mode, float lr, float beta1, float beta2, float eps, int step, double* stat_part,
                                      void* stream);

/*
 * UPA SWEEP — P UPA patch groups (UPA.py's reverse-direction loss alpha*mean(cos+1) + beta/(mean||e-l|| + 1e-3), one (alpha, beta) pair per group)
 * in ONE step. Reverse-direction UPA leaves the labels unmasked (8 labelled rows per image), so the head is the hipBLASLt GEMM — run ONCE over the
 * rows of all groups, no row limit — and K3 takes the segmented row map in VAA_LOSS_UPA mode with slice storage:
 *   vaa_loss_rows_fwd_bwd_seg_upa: vaa_loss_rows_fwd_bwd(VAA_LOSS_UPA, VAA_GRAD_SLICE) (its two launches, the same kernels) on logits [R,V] of P
 *             groups of B/P images; rowmap from vaa_loss_rowmap_build_seg, or an ordinary map with P = 1 (the bits of vaa_loss_rows_fwd_bwd).
 *             group_params host f32 [P][4] = {w, alpha, beta, scale} per group; they travel in the launch's arguments, so P <= VAA_SEG_UPA_MAX_GROUPS (else
 *             VAA_E_UNSUPPORTED). The batch means of UPA.py:375-384 run over the B/P images of a row's OWN group: the workgroup of a gradient row
 *             folds its group's statistics (the group's own map, rows and parameters — indices relative to the group) in the fixed order of the
 *             one-batch call, and the workgroup of a group's first row publishes scalars[8g .. 8g+8) and rows g*B/P .. of pred_tokens /
 *             pred_full_tokens [B, L-1]; nothing is handed over between workgroups (always two launches: VAA_K3_ONE_PASS does not apply). Group g's
 *             gradient-slice rows, scalars and prediction-map rows are bit for bit those of vaa_loss_rows_fwd_bwd on the group's logits rows alone
 *             with its ordinary map and its (alpha, beta), bf16 and fp32. Every group must label at least one row (UPA's labels are unmasked); a
 *             group without rows has no workgroup and its outputs are left as they were. grad_slice dev [R,256] in `dtype` (16-byte aligned, as
 *             logits) or NULL (evaluation: one workgroup per group); scalars dev f32 [P,8]; ws >= vaa_loss_rows_ws_bytes(R); the other arguments as
 *             vaa_loss_rows_fwd_bwd.
 *   The step ends like the target sweep's: the loss scalars are final before the backward, so vaa_step_epilogue_seg_tail carries them on the step
 *   whose scalars are read and vaa_step_epilogue_seg (zero tail) on the others; the L1 clip (UPA.py:157) needs the whole gradient's norm, so K4 is
 *   never fused into the epilogue here: vaa_patch_update_seg with l1_clip = 1e-3 follows at every world size.
 */
int vaa_loss_rows_fwd_bwd_seg_upa(const void* logits, int dtype, const void* rowmap, int R, int B, int L, int V, int P, const float* group_params,
                                  float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens, void* grad_slice, void* ws, size_t ws_bytes,
                                  void* stream);

/*
 * LM head FUSED with K3's statistics (SURVEY.md section 8f-2 as the survey wrote it; for callers that own the LM-head weight) — replaces
 * `logits = lm_head(hidden)` on the labelled rows (modeling_prismatic.py:404-415 -> HF Llama's bf16 lm_head) followed by vaa_loss_rows_stats:
 * the [R,V] logits are never written. The head weight is streamed from HBM once (full 128-byte lines, global -> LDS by LDS-DMA, into MFMA fragments), every
 * workgroup reduces its 128 vocabulary columns to per-row {max, sum exp, argmax, label logit}; a second small launch folds them per row,
 * computes the action-slice statistics (UADA.py:384-389) and — VAA_LOSS_UADA_DDP — writes the gradient slice.
 *   hidden   dev bf16 [R,D]: final-norm hidden states of the labelled rows, in the row map's order;  w_head dev bf16 [V,D]
 *   rowmap, R, B, L, V, mode, params: as vaa_loss_rows_stats;  grad_slice dev bf16 [R,256] or NULL (only VAA_LOSS_UADA_DDP)
 *   loss_ws  dev >= vaa_loss_rows_ws_bytes(R): left exactly as vaa_loss_rows_stats leaves it — vaa_step_epilogue[_update] folds it unchanged
 *   head_ws  dev >= vaa_head_loss_ws_bytes(R, V): scratch + the rows' 256 action logits (bf16) for vaa_head_loss_rows_finish;  logits_dbg dev bf16 [R,V] or NULL (tests: the bf16 logits the statistics were made of)
 * Covers vaa_head_loss_rows_applies(R, D, V) == 1: R <= 128 rows (one pass over the weight), D a multiple of 64; else VAA_E_UNSUPPORTED and the
 * caller keeps its GEMM + vaa_loss_rows_stats. Logits are the fp32 MFMA sums rounded to bf16 (the reference's bf16 head); for the same bf16
 * logits the slice statistics and the gradient slice are bit for bit those of vaa_loss_rows_stats, CE agrees to fp32 summation order.
 */
size_t vaa_head_loss_ws_bytes(int R, int V);
int vaa_head_loss_rows_applies(int R, int D, int V);
int vaa_head_loss_rows_stats(const uint16_t* hidden, const uint16_t* w_head, int D, const void* rowmap, int R, int B, int L, int V, int mode,
                             const float* params, void* grad_slice, void* loss_ws, size_t loss_ws_bytes, void* head_ws, size_t head_ws_bytes,
                             uint16_t* logits_dbg, void* stream);

/*
 * The finishing pass behind vaa_head_loss_rows_stats for callers that do not run vaa_step_epilogue: folds the rows into scalars[8] and the
 * prediction maps exactly like the second launch of vaa_loss_rows_fwd_bwd (same kernel), reading a row's 256 action logits from head_ws
 * instead of [R,V] logits — and, VAA_LOSS_UPA (UPA.py:367-387: the gradient needs the batch means), writes the gradient slice.
 * Together the two calls evaluate every mode WITHOUT logits in memory (validation passes; UADA_DDP and UPA also with their gradient);
 * the gradients of the modes with a cross-entropy term (VAA_LOSS_UADA, VAA_LOSS_CE) need every logit: VAA_E_UNSUPPORTED, use the LM-head
 * GEMM + vaa_loss_rows_fwd_bwd there.
 *   rowmap, R, B, L, V, mode, params: as given to vaa_head_loss_rows_stats;  loss_ws, head_ws: as it left them
 *   scalars dev f32[8]; pred_tokens / pred_full_tokens dev i32 [B,L-1] or NULL;  grad_slice dev bf16 [R,256] or NULL (only VAA_LOSS_UPA)
 */
int vaa_head_loss_rows_finish(const void* rowmap, int R, int B, int L, int V, int mode, const float* params, void* loss_ws, size_t loss_ws_bytes,
                              const void* head_ws, size_t head_ws_bytes, float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens,
                              void* grad_slice, void* stream);

/*
 * K3s — the SLICE-ONLY head: LM head on the labelled rows restricted to the 256 action columns + slice statistics + loss gradient + the head's
 * backward, ONE launch per inner step for the modes whose loss lives in those columns (VAA_LOSS_UADA_DDP: UADA_ddp.py:99-124; VAA_LOSS_UPA:
 * UPA.py:367-387). Replaces vaa_head_loss_rows_stats (+ finish) and the `grad_slice @ W[31744:32000]` GEMM on the steps whose full-vocabulary CE
 * and argmax nobody reads: the reference reads `celoss` once per OUTER iteration (the last inner step's value, UADA_ddp.py:214-221) and never in
 * UPA's reverse-direction mode (UPA.py:145-186), so the 263 MB weight stream runs on those steps only and this kernel (2.1 MB of weights) on all.
 *   hidden    dev bf16 [R,D];  w_head dev bf16 [V,D] (rows 31744..31999 are read);  w_slice_t dev bf16 [D,256] = the slice transposed, written
 *             ONCE per weight by vaa_head_slice_pack (frozen weights: pack at model load, keep resident); may be NULL when dhidden is NULL
 *   rowmap, R, B, L, V, mode, params: as vaa_loss_rows_stats (mode UADA_DDP or UPA, else VAA_E_UNSUPPORTED)
 *   dhidden   dev bf16 [R,D] out or NULL (forward only): d total / d hidden = g [R,256] x W[31744:32000] with g rounded to bf16 (fp32 MFMA sums)
 *   grad_slice dev bf16 [R,256] out or NULL: g itself (tests; bit for bit the slice vaa_head_loss_rows_stats / _finish write for the same rows)
 *   loss_ws   dev >= vaa_loss_rows_ws_bytes(R): the SliceStats in K3's layout and NEUTRAL full-vocabulary parts {m = -inf, s = 0}: the fold
 *             (vaa_step_epilogue[_update], or this kernel's own when scalars != NULL) then reports CE = 0 ("not evaluated on this step") and
 *             pred_full = -1; calling vaa_head_loss_rows_stats AFTERWARDS on the same loss_ws (the steps whose CE is read) replaces the parts
 *             with real ones and rewrites the same SliceStat bits
 *   scalars   dev f32[8] or NULL; pred_tokens / pred_full_tokens dev i32 [B,L-1] or NULL: folded and published by the launch itself (NULL:
 *             left to vaa_step_epilogue)
 *   ws        dev >= vaa_head_slice_ws_bytes(R): the [ceil16(R),128] action logits as 64-bit words {launch tag, logit 2q+1, logit 2q} (bf16) — the
 *             SAME MFMA sequence per element as vaa_head_loss_rows_stats (same k order), hence bit for bit its slice logits, statistics and
 *             gradient slice
 * One launch needs workgroups that wait for each other (<= 256 — 32 per block of 16 rows, 8 action columns each; VAA_K3S_COLS=16: 16 per block —; they
 * poll the tagged words they are going to use): admitted when the device keeps twice the grid resident, the stream is not being
 * captured and no other stream of the process has a waiting grid in flight; otherwise (or VAA_K3S_ONE_LAUNCH=0) the same kernel runs as two
 * launches with the same bits. A hand-over that times out NaN-poisons dhidden / the statistics AND raises vaa_async_error().
 * Covers vaa_head_slice_applies(R, D, V) == 1: R <= 128, D a multiple of 64 up to 4096, V <= 32768.
 */
int vaa_head_slice_applies(int R, int D, int V);
size_t vaa_head_slice_ws_bytes(int R);
int vaa_head_slice_pack(const uint16_t* w_head, int D, int V, uint16_t* w_slice_t, void* stream);
int vaa_head_slice_fwd_bwd(const uint16_t* hidden, const uint16_t* w_head, const uint16_t* w_slice_t, int D, const void* rowmap, int R, int B, int L,
                           int V, int mode, const float* params, uint16_t* dhidden, uint16_t* grad_slice, void* loss_ws, size_t loss_ws_bytes,
                           float* scalars, int32_t* pred_tokens, int32_t* pred_full_tokens, void* ws, size_t ws_bytes, void* stream);

/*
 * K2' (for callers that own the model's patch-embed weights) — K2 fed by the gradient of the ViT patch-embed OUTPUTS instead of the pixel gradient: the
 * patch-embed backward (modeling_prismatic.py:120-123 -> timm PatchEmbed, Conv2d(3, D, 14, stride 14) == a GEMM over 588-pixel
 * tiles) is evaluated by MFMA only for the 14x14 tiles that carry kept patch pixels and consumed in place by the gather.
 *   dy0, dy1  dev bf16 [B,256,D0], [B,256,D1]: dL/d(patch-embed output) of the DINOv2 and SigLIP towers, tokens in tile order
 *   wp0, wp1  dev bf16 [vaa_patch_embed_packed_elems(D)]: the conv weights [D,3,14,14] of a tower, flattened to [D,588], transposed to
 *             wt [588,D] and re-ordered ONCE into MFMA fragment order by vaa_patch_embed_pack_weights (frozen weights: pack at model load,
 *             keep resident; 592 x D elements — 588 columns + 4 of zero padding)
 *   keep_bits dev: K1's keep mask (required); round_bf16 != 0 rounds each tower's pixel gradient to bf16 before the 1/std scaling
 *             (what the unfused path does: the model hands back a bf16 pixel gradient); D0, D1 multiples of 64
 *   other arguments as vaa_patch_grad_gather; ws >= vaa_patch_embed_grad_ws_bytes(B, ph, pw)
 */
size_t vaa_patch_embed_packed_elems(int D);
int vaa_patch_embed_pack_weights(const uint16_t* wt, int D, uint16_t* packed, void* stream);
size_t vaa_patch_embed_grad_ws_bytes(int B, int ph, int pw);
int vaa_patch_embed_grad_gather(const uint16_t* dy0, int D0, const uint16_t* dy1, int D1, const uint16_t* wp0, const uint16_t* wp1,
                                const float* patch, const int32_t* xy, const float* theta, const uint8_t* keep_bits, int B, int ph, int pw,
                                int geometry, int mask_mode, const float* std6, int round_bf16, float* gpatch, void* ws, size_t ws_bytes,
                                void* stream);
/* the same fed by the tile-major mask of vaa_patch_apply_fwd_tiles (keep_tiles, tile_flags: both required). gpatch == NULL leaves the final
 * fixed-order sum to the caller: the vaa_patch_grad_partials(B) partial tiles [parts][3*ph*pw] f32 then sit at the start of ws. */
int vaa_patch_grad_partials(int B);
int vaa_patch_embed_grad_gather_tiles(const uint16_t* dy0, int D0, const uint16_t* dy1, int D1, const uint16_t* wp0, const uint16_t* wp1,
                                      const float* patch, const int32_t* xy, const float* theta, const uint16_t* keep_tiles,
                                      const uint32_t* tile_flags, int B, int ph, int pw, int geometry, int mask_mode, const float* std6,
                                      int round_bf16, float* gpatch, void* ws, size_t ws_bytes, void* stream);
/* the same with one patch per image (resize_patch=True; packed / pdesc / gpacked as in vaa_patch_grad_gather_multi):
 * ws >= vaa_patch_embed_grad_multi_ws_bytes(B); the resize adjoint then folds gpacked into the base patch's gradient */
size_t vaa_patch_embed_grad_multi_ws_bytes(int B);
int vaa_patch_embed_grad_gather_multi(const uint16_t* dy0, int D0, const uint16_t* dy1, int D1, const uint16_t* wp0, const uint16_t* wp1,
                                      const float* packed, const int32_t* pdesc, const int32_t* xy, const float* theta,
                                      const uint8_t* keep_bits, int B, int max_h, int max_w, int geometry, int mask_mode, const float* std6,
                                      int round_bf16, float* gpacked, void* ws, size_t ws_bytes, void* stream);
/* ... fed by the tile-major mask of vaa_patch_apply_fwd_tiles (called with pdesc) */
int vaa_patch_embed_grad_gather_multi_tiles(const uint16_t* dy0, int D0, const uint16_t* dy1, int D1, const uint16_t* wp0, const uint16_t* wp1,
                                            const float* packed, const int32_t* pdesc, const int32_t* xy, const float* theta,
                                            const uint16_t* keep_tiles, const uint32_t* tile_flags, int B, int max_h, int max_w, int geometry,
                                            int mask_mode, const float* std6, int round_bf16, float* gpacked, void* ws, size_t ws_bytes, void* stream);

/*
 * K4 — replaces transformers.AdamW.step + `patch.data.clamp(0,1)` + zero_grad (UADA.py:155-157; UADA_ddp.py:208-209),
 * optional `clip_grad_norm_([patch], l1_clip, norm_type=1)` (UPA.py:157) and the PGD sign step (TMA.py:171-175).
 *   patch,m,v dev [n] float32 in place; g dev [n] float32 (sum over ranks when grad_scale = 1/world, DDP mean); g must not alias
 *            patch, m or v (VAA_E_INVALID): several workgroups read the whole gradient while others already write their elements
 *   step     1-based Adam step count t; lr already multiplied by the cosine schedule (UADA.py:109-115,162-164)
 *   stats    dev [2] float32 out or NULL: {sum|g*grad_scale|, mean(g*grad_scale)} (the logged TRAIN_patch_gradient)
 */
int vaa_patch_update(float* patch, const float* g, float* m, float* v, int n, int mode, float lr, float beta1, float beta2,
                     float eps, int step, float l1_clip, float grad_scale, float* stats, void* stream);

/*
 * Eval-time paste — replaces RandomPatchTransform.simulation_random_patch
 * (appply_random_transform.py:43-78), called per simulator frame by the LIBERO evaluation
 * (experiments/robot/libero/run_libero_eval_args_geo_batch.py:207): patch quantised to uint8 (ToPILImage), fixed
 * rotation+shear warp when geometry[b] != 0, composite where canvas >= 0, uint8 HWC in and out. Batched over B frames.
 *   img_u8, out_u8 dev [B,224,224,3] uint8;  patch dev [3,ph,pw] float32 in [0,1];  xy dev [B,2] int32 (position);
 *   theta dev [B,6] float32 (rows 0-1 of shear_matrix(shx,shy) @ rotation_matrix(angle), :69-74);  geometry dev [B] int32
 */
int vaa_patch_apply_eval(const uint8_t* img_u8, const float* patch, const int32_t* xy, const float* theta, const int32_t* geometry,
                         int B, int ph, int pw, uint8_t* out_u8, void* stream);

/*
 * K7 — the evaluation's image front end behind the eval-time paste: replaces, per camera frame, the centre crop of get_vla_action
 * (experiments/robot/openvla_utils.py:132-155: convert_image_dtype(float32), crop_and_resize :81-124, clip_by_value,
 * convert_image_dtype(uint8, saturate=True)) and the processor call behind it (:166: to [0,1], one normalisation per vision tower, six channels,
 * bfloat16). One launch per batch; a frame's result does not depend on the batch around it.
 *   img_u8   dev  [B,224,224,3] uint8 HWC (4-byte aligned)
 *   crop_scale    0 = no crop (the frame's own bytes are normalised); else the AREA share of the centre crop, in (0, 1] (the reference: 0.9)
 *   mean6/std6 host [6] float32, as vaa_patch_apply_fwd
 *   out_bf16 dev  [B,6,224,224] bfloat16 bits (16-byte aligned): the model's pixel_values
 * VAA_E_INVALID before any launch: crop_scale negative, above 1 or NaN; B < 0; a null pointer or a misaligned one (B > 0). B == 0 returns VAA_OK
 * and launches nothing.
 * The arithmetic is the contract: TensorFlow's CPU CropAndResize (bilinear, extrapolation value 0) followed by convert_image_dtype, restated
 * with every operation a separately rounded fp32 operation (no FMA). N = 224. On the host:
 *     s = min(max(sqrtf(crop_scale), 0), 1);   y1 = x1 = (1 - s) / 2;   y2 = x2 = y1 + s;   scale = ((y2 - y1) * 223) / 223
 * Per output row y (columns alike, with x, lx, left = floor, right = ceil):
 *     in_y = y1*223 + y*scale;   t = floorf(in_y);   b = ceilf(in_y);   ly = in_y - t;     in_y or in_x outside [0, 223]: value 0 in all channels
 * Per channel, with f(u8) = (float)u8 * (1.0f / 255.0f) of the four source bytes tl, tr (row t) and bl, br (row b):
 *     top = tl + (tr - tl)*lx;   bot = bl + (br - bl)*lx;   v = top + (bot - top)*ly;   v = min(max(v, 0), 1)
 *     q = min(255, (int)(v * 255.5f))                      (truncation, as convert_image_dtype(saturate=True) does)
 * and q is normalised exactly as vaa_patch_apply_fwd normalises a frame byte: x = (float)q / 255.0f, (x - mean[c]) / std[c] with true divisions,
 * round-to-nearest-even to bfloat16, for c and c + 3. With crop_scale == 0, q is the source byte itself.
 */
int vaa_eval_preprocess(const uint8_t* img_u8, int B, float crop_scale, const float* mean6, const float* std6, uint16_t* out_bf16, void* stream);

/*
 * K8 — the resize of a simulator's camera frames to 224x224 in front of the eval-time paste: replaces, per camera frame,
 * `tf.image.resize(img, (224,224), method="lanczos3", antialias=True)` followed by round, clip_by_value(0, 255) and the uint8 cast
 * (experiments/robot/libero/libero_utils.py:44-45, experiments/robot/bridge/bridgev2_utils.py:112) and, with rot180, LIBERO's `img[::-1, ::-1]`
 * in front of it (libero_utils.py:56). One launch per batch; a frame's bytes do not depend on the batch around it; same arguments, same bits.
 *   src_u8   dev  [B,H,W,3] uint8 HWC (4-byte aligned), 8 <= H, W <= 2048
 *   rot180   0 or 1: the source is read as src[b, H-1-r, W-1-j] wherever the rules below say src[b, r, j] (no extra pass)
 *   start_x, w_x, Tx / start_y, w_y, Ty   host: the separable filter per axis (x: along W, y: along H), for each of the 224 output indices i
 *            start[i]  int32: the first source index; w[i*T + t] float32, t < T: the weight of source index start[i] + t (zero-padded to T).
 *            1 <= T <= VAA_FRAME_RESIZE_MAX_TAPS; every start[i] >= 0 and start[i] + T - 1 <= axis length - 1; every weight finite.
 *   taps_dev dev  the same four tables on the device, vaa_frame_resize_taps_bytes(Tx, Ty) bytes (4-byte aligned), packed in the order
 *            int32 start_x[224], int32 start_y[224], float32 w_x[224*Tx], float32 w_y[224*Ty]. The host tables are what is validated, the
 *            device copy is what the kernel reads; the kernel clamps every source index to the axis, so a device copy that differs from
 *            the validated tables cannot read outside src.
 *   dst_u8   dev  [B,224,224,3] uint8 HWC (16-byte aligned): the layout vaa_patch_apply_eval takes
 * Before any launch: B < 0 or (B > 0) a NULL pointer, rot180 not 0 / 1, T < 1, a start outside the axis or a non-finite weight: VAA_E_INVALID;
 * B == 0: VAA_OK, nothing is read or written; H or W outside [8, 2048], T > VAA_FRAME_RESIZE_MAX_TAPS, a misaligned base: VAA_E_UNSUPPORTED.
 *
 * The arithmetic is the contract: fp32 throughout, every operation separately rounded (no FMA), the horizontal pass first, the taps of a
 * pass accumulated in ascending source index starting from 0.0f. With p(r, j, c) = (float)src[b, r, j, c] (after rot180):
 *     h(r, x, c) = (..((0 + w_x[x][0] * p(r, sx, c)) + w_x[x][1] * p(r, sx + 1, c)) + ..) + w_x[x][Tx-1] * p(r, sx + Tx - 1, c),  sx = start_x[x]
 *     v(y, x, c) = (..((0 + w_y[y][0] * h(sy, x, c)) + w_y[y][1] * h(sy + 1, x, c)) + ..) + w_y[y][Ty-1] * h(sy + Ty - 1, x, c),  sy = start_y[y]
 *     dst[b, y, x, c] = (uint8) min(max(rintf(v), 0), 255)             (rintf: round half to even, as tf.round)
 *
 * The tables are the caller's; the ones the evaluation uses (resize.lanczos3_taps) follow TensorFlow's ScaleAndTranslate rule for
 * lanczos3 with antialias. THE RULE IS WRITTEN HERE FROM MEMORY: TensorFlow cannot be run on this platform, so neither the span, nor the
 * normalisation, nor the rounding of the weights could be compared with it — this header is the definition. Per axis, in -> out = 224,
 * everything in fp64:
 *     scale = in / out;   kernel_scale = max(scale, 1);   T = 2*ceil(3*kernel_scale) + 1
 *     sample point of output index i (pixel-edge coordinates):  s = (i + 0.5) * scale
 *     span: lo = max(ceil(s - 3*kernel_scale - 0.5), 0),  hi = min(floor(s + 3*kernel_scale - 0.5), in - 1)     (at most T indices)
 *     raw weight of source index j in [lo, hi]:  L((j + 0.5 - s) / kernel_scale),   L(x) = sinc(x) * sinc(x / 3) on |x| < 3, else 0,
 *         sinc(x) = sin(pi*x) / (pi*x), sinc(0) = 1
 *     the raw weights of a span are divided by their sum (added in ascending j), then rounded to fp32
 *     start = max(min(lo, in - T), 0): the window of T indices is shifted into the axis at its end; positions outside [lo, hi] hold 0
 */
#define VAA_FRAME_RESIZE_MAX_TAPS 57 /* 2*ceil(3*2048/224) + 1 */
size_t vaa_frame_resize_taps_bytes(int Tx, int Ty);
int vaa_frame_resize(const uint8_t* src_u8, int B, int H, int W, int rot180, const int32_t* start_x, const float* w_x, int Tx,
                     const int32_t* start_y, const float* w_y, int Ty, const void* taps_dev, uint8_t* dst_u8, void* stream);

/*
 * K9 — the evaluation's crop (K7's geometry) sampled inside a training step: crop + bilinear resize back to 224x224 of K1's planar pixel
 * values with one box per image, and the adjoint that carries the model's pixel gradient back in front of K2. It acts on the normalised
 * bf16 planes, not on the uint8 frame: normalisation is affine per channel and the bilinear taps sum to 1, so cropping after it equals
 * normalising after the crop up to rounding. One launch per call; an image's result does not depend on the batch around it; same arguments,
 * same bits (the adjoint is a gather per source element, no atomics).
 *   x_bf16 / gout_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned)
 *   boxes_host, boxes_dev     [B,4] float32 {y1, x1, y2, x2} in crop_and_resize's normalised coordinates, on the host and (16-byte aligned)
 *            on the device. The host copy is what is validated, the device copy is what the kernels read; the kernels clamp every index
 *            to the frame, so a device copy that differs from the validated boxes cannot read or write outside the tensors.
 *   out_bf16 / gx_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned). Every element is written (the caller never zeroes gx).
 * VAA_E_INVALID before any launch: B < 0; with B > 0 a NULL pointer, a misaligned device base, or a box with a coordinate that is not
 * finite or breaks 0 <= y1 < y2 <= 1, y2 - y1 >= 0.5 (fp32 difference) or the same along x. B == 0 returns VAA_OK and launches nothing.
 *
 * The forward arithmetic is the contract: fp32, every operation separately rounded (no FMA), K7's own expressions per image and axis
 * (columns alike, with x1, x2, x, lx, left = floor, right = ceil):
 *     org_y = y1*223;   scale_y = ((y2 - y1)*223)/223
 *     in_y = min(max(org_y + y*scale_y, 0), 223);   t = floorf(in_y);   b = ceilf(in_y);   ly = in_y - t
 * The clamp stands where K7 has "outside [0, 223] -> 0"; with a valid box it can only fire through rounding when y2 == 1. Per channel c < 6,
 * with the four source values widened to fp32, tl, tr from row t and bl, br from row b (columns left, right):
 *     top = tl + (tr - tl)*lx;   bot = bl + (br - bl)*lx;   v = top + (bot - top)*ly;   out[b,c,y,x] = bf16(v)  (round to nearest even)
 * The box {0,0,1,1} returns its input bit for bit for finite inputs (a negative zero comes back as +0: x + 0*0).
 *
 * The adjoint is the exact transpose of those taps. With t, b, ly of output row y as above, the weight of y on source row r is
 *     wy(y, r) = [t(y) == r]*(1 - ly(y)) + [b(y) == r]*ly(y)        (a row that is both gets (1 - 0) + 0 = 1)
 * and wx(x, j) alike. An output index TOUCHES a source index when its t or its b equals it; its weight is then never 0. Then
 *     gx[b,c,r,j] = bf16( sum_y wy(y, r) * ( sum_x wx(x, j) * gout[b,c,y,x] ) )
 * over the touching y and x only, both sums starting from 0.0f with ascending indices, every product and every add a separately rounded fp32
 * operation, one rounding to bf16 at the end. A source element that no output touches is written as +0. Which outputs touch an index is
 * decided by evaluating the forward's own t and b for each candidate (the candidates of j are the six indices from
 * floor((j - org)/scale) - 2: a side of at least 0.5 puts every touching output among them), never by a second formula.
 *
 * What K9 does not model: K5's uint8 quantisation of the patch, K7's uint8 truncation of the cropped frame, and the
 * order of interpolation and bf16 rounding (K9 interpolates values K1 has already rounded).
 */
int vaa_crop_resize_fwd(const uint16_t* x_bf16, const float* boxes_host, const float* boxes_dev, int B, uint16_t* out_bf16, void* stream);
int vaa_crop_resize_bwd(const uint16_t* gout_bf16, const float* boxes_host, const float* boxes_dev, int B, uint16_t* gx_bf16, void* stream);

/*
 * K10 — scene-lighting jitter of the pasted frame inside a training step: brightness, contrast, saturation and hue of the WHOLE frame (patch
 * and surroundings together), one factor row per image, on K1 / K9's planar pixel values, and its adjoint. It is the photometric half of
 * OpenVLA's `image_aug` (prismatic/vla/datasets/datasets.py:126-138: random brightness 0.2, contrast and saturation 0.8-1.2, hue 0.05, behind the
 * 0.9 random crop, which is K9). TensorFlow / dlimp do not exist on this platform: what follows is THIS PROJECT'S OWN STATEMENT of that
 * augmentation (additive brightness, a contrast mean per channel, a YIQ hue rotation) and is not pinned against tf.image; as for K0c and K9
 * this header is the definition.
 *   x_bf16 / gout_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned). Channels 0-2 (mean6 / std6 entries 0-2) and 3-5 (entries 3-5) are
 *            two RGB images — the two towers' normalisations of one frame — processed independently with the same factors.
 *   factors_host, factors_dev  [B,12] float32 {delta, kappa, sigma, R[0][0..2], R[1][0..2], R[2][0..2]} on the host and (16-byte aligned) on the
 *            device. The host copy is what is validated, the device copy is what the kernels read; no address depends on a factor, so a
 *            device copy that differs from the validated one changes values only.
 *   mean6, std6          host [6] float32, the normalisation K1 applied
 *   out_bf16 / gx_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned). Every element is written (the caller never zeroes gx).
 *   ws, ws_bytes         dev  scratch of at least vaa_scene_jitter_ws_bytes(B) bytes, 8-byte aligned: the per-part partial sums
 * VAA_E_INVALID before any launch: B < 0 (or beyond the grid: B > (2^31 - 1)/28); with B > 0 a NULL pointer, a misaligned device base, a mean
 * or std that is not finite, std_c <= 0, a factor that is not finite, kappa < 0 or sigma < 0. VAA_E_WORKSPACE before any launch: ws NULL,
 * misaligned or too small. B == 0 returns VAA_OK and launches nothing.
 *
 * R is the hue rotation by h turns, built by the caller in fp64 and rounded to fp32:
 *     R(h) = I + Tinv * (rot(2*pi*h) - I) * T,     rot(a) = [[1, 0, 0], [0, cos a, -sin a], [0, sin a, cos a]]
 *     T = [[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]]   (RGB -> YIQ; Tinv its fp64 inverse)
 * It is exactly the identity for h = 0 (rot - I is exactly 0), and every row sums to 1 (T maps gray to (1, 0, 0), which rot leaves alone).
 *
 * The forward arithmetic is the contract. Per image and tower, with N = 224*224, fp32, every a*b + c below ONE FMA on a rounded c:
 *     p_c    = fma(x_c, std_c, mean_c)                                               back to pixel space
 *     pre1_c = p_c + delta;                             y1_c = clamp(pre1_c, 0, 1)   brightness
 *     m_c    = fp32( (sum over the pixels of y1_c) / N )                             one mean PER CHANNEL; the sum and the division in fp64
 *     pre2_c = fma(kappa, y1_c, (1 - kappa)*m_c);       y2_c = clamp(pre2_c, 0, 1)   contrast
 *     gray   = fma(0.114, y2_B, fma(0.587, y2_G, 0.299*y2_R))                        K0c's
 *     pre3_c = fma(sigma, y2_c, (1 - sigma)*gray);      y3_c = clamp(pre3_c, 0, 1)   saturation
 *     pre4_c = fma(R[c][2], y3_B, fma(R[c][1], y3_G, R[c][0]*y3_R));  y4_c = clamp(pre4_c, 0, 1)   hue
 *     out_c  = bf16( (y4_c - mean_c) / std_c )                                       true division, round to nearest even
 * 1 - kappa and 1 - sigma are fp32 differences. clamp is torch.clamp (x < 0 ? 0 : x > 1 ? 1 : x): a NaN in x stays a NaN, and makes m_c — so
 * that whole plane of that image — a NaN. The sum for m_c has a fixed order: a plane is 14 parts of 448 runs of 8 consecutive elements; a run
 * is added in ascending order, the 448 runs of a part by a butterfly over 64 runs (xor 32, 16, ..., 1) and then the 7 groups of 64 in
 * ascending order, the 14 parts in ascending order, all in fp64. The identity factors (0, 1, 1, I) give out_c = bf16((clamp(p_c) - mean_c)/std_c).
 *
 * The adjoint is the exact derivative with torch.clamp's gate at each of the four clamps (the gradient passes where 0 <= pre <= 1, bounds
 * included, never for a NaN), the gates recomputed from x and the factors (nothing of the forward is kept; the means are summed again):
 *     G4_c = gate(pre4_c) ? gout_c * fp32(1/std_c) : 0                               1/std_c rounded from fp64, as K2 applies it
 *     G3_d = gate(pre3_d) ? fma(R[2][d], G4_B, fma(R[1][d], G4_G, R[0][d]*G4_R)) : 0 the transposed matrix
 *     G2_c = gate(pre2_c) ? fma(sigma, G3_c, ((1 - sigma)*w_c) * ((G3_R + G3_G) + G3_B)) : 0        w = (0.299, 0.587, 0.114)
 *     s_c  = fp32( (sum over the pixels of G2_c) / N )                               the whole-image term of the contrast mean, per channel,
 *                                                                                    summed in the order of m_c
 *     G1_c = gate(pre1_c) ? fma(kappa, G2_c, (1 - kappa)*s_c) : 0
 *     gx_c = bf16( G1_c * std_c )
 * Launches: forward 2 (part sums of y1; apply), adjoint 3 (part sums of y1; part sums of G2; apply), each B*2*14 workgroups whatever the
 * factors. No atomics; an image's result does not depend on the batch around it; the same arguments give the same bits.
 */
size_t vaa_scene_jitter_ws_bytes(int B);
int vaa_scene_jitter_fwd(const uint16_t* x_bf16, const float* factors_host, const float* factors_dev, const float* mean6, const float* std6, int B,
                         uint16_t* out_bf16, void* ws, size_t ws_bytes, void* stream);
int vaa_scene_jitter_bwd(const uint16_t* gout_bf16, const uint16_t* x_bf16, const float* factors_host, const float* factors_dev, const float* mean6,
                         const float* std6, int B, uint16_t* gx_bf16, void* ws, size_t ws_bytes, void* stream);

/*
 * K11 — camera defocus blur of the pasted frame inside a training step: a separable 13-tap low-pass with edge replication, one tap row per
 * image, on K1's planar pixel values (in front of K9 and K10: optics act before the crop), and its adjoint. The blur is linear and its taps
 * sum to 1, so it commutes with the per-channel affine normalisation up to rounding: like K9 it acts on the normalised bf16 planes and needs
 * no mean6 / std6. One launch per call; an image's result does not depend on the batch around it; same arguments, same bits (the adjoint is a
 * gather per source element: no atomics, no workspace).
 *   x_bf16 / gout_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned)
 *   taps_host, taps_dev       [B,8] float32 rows {w0, w1, ..., w6, 0} on the host and (16-byte aligned) on the device. The 13-tap kernel of
 *            image b is w_|t|, t = -6..6, the same along both axes and for all six planes. The host copy is what is validated, the device
 *            copy is what the kernels read; no address depends on a tap, so a device copy that differs changes values only.
 *   out_bf16 / gx_bf16   dev  [B,6,224,224] bfloat16 bits (16-byte aligned). Every element is written (the caller never zeroes gx). The
 *            input and the output must not overlap (checked by address ranges: a workgroup reads rows that its neighbours write).
 * VAA_E_INVALID before any launch: B < 0, or B > (2^31 - 1)/42 = 51130563 (the grid: one workgroup per image, plane and band of 32 rows); with
 * B > 0 a NULL pointer, a misaligned device base, overlapping buffers, a tap that is not finite or is below 0, w0 <= 0, row[7] != 0, or
 * w0 + 2*(w1 + ... + w6), summed in fp64, further than 1e-5 from 1. B == 0 returns VAA_OK and launches nothing.
 *
 * The forward arithmetic is the contract: fp32, every product and every add a separately rounded operation (no FMA), both sums from 0.0f with
 * t ascending. With c(i) = min(max(i, 0), 223) (edge replication: the camera sees more scene beyond the frame, not black), per plane:
 *     h[y,x]   = sum over t = -6..6 of  w_|t| * x[y, c(x+t)]          kept in fp32
 *     v[y,x]   = sum over t = -6..6 of  w_|t| * h[c(y+t), x]
 *     out[y,x] = bf16(v[y,x])                                         round to nearest even
 * The taps (1,0,0,0,0,0,0,0) return their input bit for bit for finite inputs (a negative zero comes back as +0).
 *
 * The adjoint is the exact transpose of V*H, the edge accumulation included:
 *     a[r,x]  = sum over y ascending, within it t = -6..6 ascending, of  [c(y+t) == r] * w_|t| * g[y,x]          kept in fp32
 *     gx[r,j] = bf16( sum over x ascending, within it t ascending, of  [c(x+t) == j] * w_|t| * a[r,x] )
 * over the terms whose bracket is 1, from 0.0f, every product and add separately rounded. An interior index gets at most 13 terms (t = r - y);
 * index 0 collects from output i every t with i + t <= 0, index 223 every t with i + t >= 223.
 */
int vaa_defocus_blur_fwd(const uint16_t* x_bf16, const float* taps_host, const float* taps_dev, int B, uint16_t* out_bf16, void* stream);
int vaa_defocus_blur_bwd(const uint16_t* gout_bf16, const float* taps_host, const float* taps_dev, int B, uint16_t* gx_bf16, void* stream);

/*
 * K12 — the JPEG round trip of a simulator's camera frames in front of K8: what the pixels of a frame are after a baseline JPEG encoder
 * and decoder of the libjpeg family, without the file. The reference's resize_image (experiments/robot/libero/libero_utils.py:42-43)
 * encodes every frame with tf.io.encode_jpeg and decodes it again before the lanczos3 resize ("as done in RLDS dataset builder"). Huffman
 * coding, markers and the bit stream are lossless, so only the lossy chain is computed: colour conversion, 4:2:0 subsampling, 8x8 forward
 * DCT, quantise, dequantise, inverse DCT, chroma upsampling, colour conversion back. No coefficient is ever written to memory.
 * TensorFlow does not exist on this platform. tf.image.encode_jpeg's defaults are stated FROM MEMORY AND ARE UNVERIFIED: quality 95, chroma
 * subsampling on (4:2:0), baseline, and decode_image with the default ("slow") integer IDCT and fancy upscaling. They are the settings
 * that Pillow's save(format="JPEG", quality=95, subsampling=2) followed by a load selects; tests/golden/jpeg_pillow.npz records what
 * Pillow 12.2 / libjpeg-turbo 3.1 makes of a few frames, and the arithmetic below reproduces every recorded byte.
 *   src_u8   dev  [B,H,W,3] uint8 HWC (4-byte aligned), 8 <= H, W <= 2048: K8's layout and range
 *   rot180   0 or 1: the frame that is encoded is src[b, H-1-y, W-1-x] (LIBERO rotates first, then encodes; K8 then runs with rot180 = 0)
 *   qtab_host, qtab_dev   [2][64] uint16 quantisation tables {luminance, chrominance} in natural (row-major) order, entries 1..255, on the
 *            host and (2-byte aligned) on the device. The host copy is what is validated, the device copy is what the kernels read; no
 *            address depends on an entry (a zero in a differing device copy divides by 1).
 *   dst_u8   dev  [B,H,W,3] uint8 HWC (4-byte aligned). Every byte is written. src and dst must not overlap (checked by address ranges).
 *   ws, ws_bytes  dev  scratch of at least vaa_jpeg_roundtrip_ws_bytes(B, H, W) = B*2*(8*MY)*(8*MX) bytes, 8-byte aligned: the decoded
 *            half-resolution chroma planes [B][2][8*MY][8*MX] uint8, MX = ceil(W/16), MY = ceil(H/16). vaa_jpeg_roundtrip_ws_bytes returns 0
 *            for sizes the call refuses.
 * VAA_E_INVALID before any launch: B < 0 or beyond the grid (B*MY*ceil(MX/8) > 2^31 - 1); with B > 0 H or W outside [8, 2048], rot180 not
 * 0 / 1, a NULL or misaligned pointer, overlapping src and dst, a table entry outside 1..255. VAA_E_WORKSPACE before any launch: ws NULL,
 * misaligned or too small. B == 0 returns VAA_OK and launches nothing. Two launches (chroma; luminance + finish), no atomics; an image's
 * result does not depend on the batch around it; the same arguments give the same bits.
 *
 * The arithmetic is the contract: int32 throughout, >> is the arithmetic shift (floor), FIXn(x) = (int)(x * 2^n + 0.5),
 * DESCALE(v, n) = (v + 2^(n-1)) >> n. It follows libjpeg's sample converters and its default ("slow integer") DCT pair, restated here
 * because libjpeg's sources are not part of this project: THIS HEADER IS THE DEFINITION.
 *
 * 1. Colour (encoder), per pixel of the (rotated) frame, F = FIX16:
 *     Y  = ( F(.29900)*R + F(.58700)*G + F(.11400)*B + 32768) >> 16
 *     Cb = (-F(.16874)*R - F(.33126)*G + F(.50000)*B + (128 << 16) + 32767) >> 16
 *     Cr = ( F(.50000)*R - F(.41869)*G - F(.08131)*B + (128 << 16) + 32767) >> 16
 * 2. Padding and 4:2:0 subsampling. The frame is covered by MY x MX MCUs of 16x16 pixels. Y(y, x) beyond the frame is Y(min(y, H-1),
 *    min(x, W-1)). The half-resolution planes have ch = ceil(H/2) real rows; sample (i, j), i < 8*MY, j < 8*MX, with i' = min(i, ch - 1)
 *    (the encoder replicates the last SUBSAMPLED row, so with an even H the padding rows average the last two frame rows), is
 *     C(i, j) = (c(y0, x0) + c(y0, x1) + c(y1, x0) + c(y1, x1) + bias) >> 2,   bias = 1 for even j, 2 for odd j,
 *     y0 = min(2i', H-1), y1 = min(2i'+1, H-1), x0 = min(2j, W-1), x1 = min(2j+1, W-1)
 * 3. Forward DCT of every 8x8 block on d = sample - 128, rows first, then columns; the result is 8 x the DCT. With the constants
 *    c298 = 2446, c390 = 3196, c541 = 4433, c765 = 6270, c899 = 7373, c1175 = 9633, c1501 = 12299, c1847 = 15137, c1961 = 16069, c2053 = 16819,
 *    c2562 = 20995, c3072 = 25172 (FIX13 of 0.298631336 ... 3.072711026), one eight-point pass on d0..d7 is
 *     t0 = d0+d7, t7 = d0-d7, t1 = d1+d6, t6 = d1-d6, t2 = d2+d5, t5 = d2-d5, t3 = d3+d4, t4 = d3-d4
 *     t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2
 *     o0 = (t10+t11) << 2, o4 = (t10-t11) << 2 in the row pass;   o0 = DESCALE(t10+t11, 2), o4 = DESCALE(t10-t11, 2) in the column pass
 *     z1 = (t12+t13)*c541;   o2 = DESCALE(z1 + t13*c765, n);   o6 = DESCALE(z1 - t12*c1847, n)       n = 11 (rows), 15 (columns)
 *     z1 = t4+t7, z2 = t5+t6, z3 = t4+t6, z4 = t5+t7, z5 = (z3+z4)*c1175
 *     t4 *= c298, t5 *= c2053, t6 *= c3072, t7 *= c1501;   z1 *= -c899, z2 *= -c2562, z3 = z3*(-c1961) + z5, z4 = z4*(-c390) + z5
 *     o7 = DESCALE(t4+z1+z3, n), o5 = DESCALE(t5+z2+z4, n), o3 = DESCALE(t6+z2+z3, n), o1 = DESCALE(t7+z1+z4, n)
 * 4. Quantise by division, rounding half away from zero, and dequantise, with q the table entry (luminance for Y, chrominance for Cb, Cr):
 *     k = sign(o) * ((|o| + 4*q) / (8*q))  (truncating division);    v = k*q
 * 5. Inverse DCT, columns first (n = 11), then rows (n = 18), one eight-point pass on v0..v7:
 *     z1 = (v2+v6)*c541;   t2 = z1 - v6*c1847;   t3 = z1 + v2*c765;   t0 = (v0+v4) << 13;   t1 = (v0-v4) << 13
 *     t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2
 *     u0 = v7, u1 = v5, u2 = v3, u3 = v1;   z1 = u0+u3, z2 = u1+u2, z3 = u0+u2, z4 = u1+u3, z5 = (z3+z4)*c1175
 *     u0 *= c298, u1 *= c2053, u2 *= c3072, u3 *= c1501;   z1 *= -c899, z2 *= -c2562, z3 = z3*(-c1961) + z5, z4 = z4*(-c390) + z5
 *     u0 += z1+z3, u1 += z2+z4, u2 += z2+z3, u3 += z1+z4
 *     o0, o7 = DESCALE(t10 +- u3, n);  o1, o6 = DESCALE(t11 +- u2, n);  o2, o5 = DESCALE(t12 +- u1, n);  o3, o4 = DESCALE(t13 +- u0, n)
 *    and the decoded sample is min(max(o + 128, 0), 255).
 * 6. "Fancy" chroma upsampling of the decoded half-resolution plane D, real size ch x cw = ceil(H/2) x ceil(W/2) (what lies beyond is never
 *    read: the edges are those of the frame, not of the MCUs), the 3:1 triangle filter vertically, then horizontally. For pixel (y, x) with
 *    i = y >> 1, j = x >> 1:   i2 = max(i-1, 0) for even y, min(i+1, ch-1) for odd y;   s(j) = 3*D(i, j) + D(i2, j)
 *     even x:  c = (3*s(j) + s(max(j-1, 0)) + 8) >> 4;        odd x:  c = (3*s(j) + s(min(j+1, cw-1)) + 7) >> 4
 * 7. Colour (decoder), F = FIX16, cb = Cb - 128, cr = Cr - 128, each result clamped to 0..255:
 *     R = Y + ((F(1.40200)*cr + 32768) >> 16);   G = Y + ((-F(.34414)*cb + 32768 - F(.71414)*cr) >> 16);   B = Y + ((F(1.77200)*cb + 32768) >> 16)
 */
size_t vaa_jpeg_roundtrip_ws_bytes(int B, int H, int W);
int vaa_jpeg_roundtrip(const uint8_t* src_u8, int B, int H, int W, int rot180, const uint16_t* qtab_host, const uint16_t* qtab_dev,
                       uint8_t* dst_u8, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAA_H_ */
