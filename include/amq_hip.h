/* amq_hip.h -- C ABI of libamq_hip.so: the MI355X (gfx950) replacement for the
 * native kernels on AMQ's mixed-precision inference hot path.
 *
 * What it replaces (reference paths relative to the dlwns147/amq checkout):
 *   pybind module `auto_gptq`          amq/kernel/AutoGPTQ/auto_gptq_kernel.cu:471-475
 *       vecquant{2,3,4}matmul_faster_old(vec, mat, mul, scales, zeros, groupsize, vec_height)
 *   pybind module `faster_transformer` amq/kernel/ft/FT.cpp:9-19
 *       gemv_4bit(x, kernel, scales, scaled_zeros, m, n, k, group_size)   gemv_cuda.cu:358-525
 *       gemm_4bit(x, kernel, scales, scaled_zeros)                        gemm_cuda.cu:929-1033
 *   host packers  GPTQLinear.pack (hqq/backends/autogptq.py:111-156),
 *                 pack_intweight  (hqq/backends/ft.py:15-55)
 *   dequantize    Quantizer.dequantize (hqq/core/quantize.py:184-199)
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t
 *     passed as void* (NULL = default stream).  All work is stream-ordered and
 *     asynchronous; nothing allocates, synchronises or touches global state,
 *     so every call may be captured into a hipGraph.
 *   - every pointer is a DEVICE pointer owned by the caller unless noted.
 *   - return value: AMQ_OK (0) or a negative AMQ_E* code; amq_last_error()
 *     returns a thread-local message for the most recent failure.
 *   - fp16 activations / outputs, fp32 accumulation; weights 2, 3 or 4 bit,
 *     group size 128 along K (what AMQ produces: amq/amq_quantization_proxy.py:22,36) or a multiple of 128 that divides K: the
 *     `group` argument of the amq_repack_from_* / amq_dequantize_hqq_f16 calls is the SOURCE format's group size (HQQ's packing
 *     geometry depends on it); each group's (scale, zero) is replicated into the native layout's per-128 pairs, so the compute
 *     entry points are the same kernels for every such group size.  Groups of 64 and 32 (HQQ's default group_size is 64,
 *     hqq/core/quantize.py:1078; the reference's GPTQ kernels take any groupsize, auto_gptq_kernel.cu:203) keep 128 / group pairs per
 *     (row, 128-column tile) in the native meta (amq_native_meta_bytes grows accordingly) and are served by: the amq_repack_from_* and
 *     amq_dequantize_* calls, the GEMV kernel (amq_gemv_f16 / amq_gemv_grouped_f16: <= 16 rows, every prologue, default options), the few-row
 *     GEMM up to 256 rows and the tiled GEMM beyond (amq_gemm_f16; AMQ_GEMM_AUTO / _SKINNY / _TILED of the route
 *     calls) and, for launches that fill 256 x 256 tiles, the dequantize-once GEMM route (amq_gemm_route_f16 / amq_gemm_res_f16 /
 *     amq_gemm_gated_f16 with the amq_gemm_route_workspace_bytes_g workspace); the ring / wave-specialised routes and the other compute
 *     entry points return an error for them.  The compute calls' `group` argument is therefore the
 *     NATIVE buffers' granularity: 64, 32, or anything >= 128.  N % 16 == 0, K % 128 == 0.
 *   - "native" buffers are in the AMQ-T16 layout (amq_common.cuh);
 *     sizes from amq_native_*_bytes(); produced by the amq_repack_from_* calls.
 */
#ifndef AMQ_HIP_H
#define AMQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMQ_VERSION 521            /* 0.5.2: the per-sequence step-state entry points (amq_*_seq_f16) added, nothing else changed (additions keep the number).
                                    * amq_gemv_route / amq_gemv_segment_order and the value AMQ_GEMV_DEPTH_GENERIC of amq_gemv_opts.depth added, nothing else changed.
                                    * LAYOUT CHANGE under the same number: amq_gemv_opts gained a trailing field, act_mask (and AMQ_PRO_MUL was added).  A caller that
                                    * passes a non-NULL amq_gemv_opts must be rebuilt against this header -- the library reads six ints; NULL opts are unaffected.
                                    * amq_rope_table_freqs_f16 (rope_scaling) and amq_decode_tail_suppress_f16 added, nothing else changed.  0.5.1: the bfloat16 entry points
                                    * (amq_*_bf16) added.  0.5.0: amq_gemv_opts.math renumbered
                                    * (0 = the build's default), amq_default_gemv_math added; the decode-engine and fused q/k/v-attention entry points live in
                                    * libamq_hip_ab.so (include/amq_hip_ab.h) since 0.4 */

#define AMQ_OK            0
#define AMQ_EINVAL       -1        /* bad argument (null pointer, bits, mode ...) */
#define AMQ_ESHAPE       -2        /* unsupported shape (N % 16, K % 128, group not 32 / 64 / a multiple of 128 dividing K, M out of range) */
#define AMQ_ELAUNCH      -3        /* HIP launch failed (message carries hipGetErrorString) */
#define AMQ_EUNSUPPORTED -4        /* valid request this build does not implement */

/* dequantisation arithmetic carried by a native buffer's meta */
#define AMQ_MODE_HQQ 0             /* meta = (scale, zero):  w = fp16(fp16(q - zero) * scale)   quantize.py:198 */
#define AMQ_MODE_FMA 1             /* meta = (scale, c):     w = fp16(fma(q, scale, c))          auto_gptq_kernel.cu:206, gemv_cuda.cu:151 */
#define AMQ_MODE_FMA1 2            /* AMQ_MODE_FMA for a buffer whose scales satisfy |scale| <= amq_fma1_scale_bound(bits): the GEMV kernel then unpacks a
                                    * weight pair with one packed fma instead of two ops -- the same weights, bit for bit (the caller vouches for the bound:
                                    * larger scales overflow the pre-scaled multiplier); every other kernel treats it as AMQ_MODE_FMA */

/* fused x transforms of amq_gemv_grouped_f16 */
#define AMQ_PRO_NONE     0
#define AMQ_PRO_RMSNORM  1         /* x <- gamma * fp16(x * rsqrt(mean(x^2) + eps))   (LlamaRMSNorm; FT generalT5LayerNorm, layernorm.cu:25-51) */
#define AMQ_PRO_SILU_MUL 2         /* x <- fp16(silu(x)) * x2                           (LlamaMLP act_fn(gate) * up) */
#define AMQ_PRO_MUL      4         /* x <- x * x2: AMQ_PRO_SILU_MUL over an x that the launch which wrote it already activated (amq_gemv_opts.act_mask):
                                    * the same bits, SiLU taken once per element instead of once per workgroup and element.  Groups of 128. */

#define AMQ_MAX_SEGMENTS 4

int amq_version(void);
const char* amq_last_error(void);

/* GEMV arithmetic (MODE_HQQ buffers, whose reference dequant has two fp16 roundings per weight: quantize.py:198).
 *   EXACT      both roundings per weight, bit-identical weights to Quantizer.dequantize; x*w accumulated in fp32.
 *   GROUPSCALE (opt-in) the first rounding exactly as EXACT, d = fp16((q - z) * 2^-9); the scale is applied once per (row, 128-group) in fp32
 *              after the tile's MFMAs: y += (s * 2^9) * sum_k x_k d_k.  One fp16 rounding per weight is not taken (<= 2^-11 relative per weight):
 *              measured 3.2e-4 of rms(y) rms from the reference result, worst element 0.93 of the parity bar |dy| <= 1e-3 |y| + 1e-3 rms(y), and
 *              2 fp16 ulps -- past the bar -- on a few elements per 10^4 when a bias add rounds a second time (profiles/r05_gemv_groupscale.txt):
 *              not the default for that reason.  6.5 instead of 12 VALU cycles per weight pair: +5 % decode tokens/s on Llama-2-7B, +13 % on 70B.
 *              The reference's own CUDA kernels round once per weight too (auto_gptq_kernel.cu:206-218).  Buffers in AMQ_MODE_FMA / _FMA1 (one
 *              rounding by definition) and groups of 64 / 32 run their exact forms under it.
 *   LINEAR     no per-weight roundings at all: y = sum_g s_g * (sum_k x_k q_k - z_g sum_k x_k) in fp32 -- the real-valued dequant (opt-in;
 *              ~3.6e-4 of rms(y) rms, beyond the parity bar at its worst elements).
 *   DEFAULT    what amq_default_gemv_math() returns for this build of the library. */
#define AMQ_MATH_DEFAULT    0
#define AMQ_MATH_LINEAR     1
#define AMQ_MATH_GROUPSCALE 2
#define AMQ_MATH_EXACT      3
int amq_default_gemv_math(void);   /* AMQ_MATH_EXACT or AMQ_MATH_GROUPSCALE */

/* Per-call launch options of amq_gemv_grouped_f16 (host struct; NULL or all-zero = defaults).  There is no
 * process-wide option state in the library: what a call computes depends on its arguments only. */
typedef struct amq_gemv_opts {            /* (six ints since act_mask was added: see AMQ_VERSION) */
    int math;    /* AMQ_MATH_DEFAULT (0), _EXACT, _GROUPSCALE or _LINEAR */
    int waves;   /* A/B: waves per workgroup, 0 = auto, 4, 8 or 16 */
    int depth;   /* A/B: tile loads in flight per wave, 0 = auto, 2 or 4; AMQ_GEMV_DEPTH_GENERIC = auto, and a launch amq_gemv_route() sends to the
                  * keyed kernels runs the generic kernel instead, geometry and segment order unchanged (the same bits) */
    int rpt;     /* A/B: row-tiles walked by one workgroup, 0 = auto, 1..64 */
    int dot;     /* A/B: 1 = M == 1 runs the v_dot2c + wavefront-shuffle body instead of the MFMA body */
    int act_mask; /* bit i: segment i stores y = fp16(silu(x W^T + bias)) -- gate_proj, for a consumer with AMQ_PRO_MUL.  Not with a residual on that
                   * segment; groups of 128 */
} amq_gemv_opts;
#define AMQ_GEMV_DEPTH_GENERIC (-1)

/* Which GEMV kernel amq_gemv_grouped_f16 launches for these arguments -- a host-side function of them alone, no device needed.
 *   AMQ_GEMV_ROUTE_KEYED    kernels with the segments' bit-widths fixed at compile time (no per-workgroup dispatch on a key): the one-row launches of a
 *                           7B-class decode step.  All of: M == 1, groups of 128 (or multiples), exact math, every segment AMQ_MODE_HQQ, opts.depth,
 *                           opts.rpt and opts.dot zero, and AMQ_PRO_RMSNORM with 1 .. 3 segments or AMQ_PRO_NONE with one on 8 waves at K <= 4096, or
 *                           AMQ_PRO_MUL / AMQ_PRO_SILU_MUL with one segment on 16 waves at K <= 16384.  The waves are opts.waves, or what the launch
 *                           picks itself: 8 for 2048 <= K <= 4096, 16 beyond.
 *   AMQ_GEMV_ROUTE_GENERIC  the kernel that holds every (bits, mode) body: everything else, and opts.depth == AMQ_GEMV_DEPTH_GENERIC.
 * Both compute the same bits.  A launch of the keyed geometry (forced generic or not) runs its segments in ascending bit-width:
 * amq_gemv_segment_order() gives that order (order[i] = index of the segment launched i-th; equal widths keep the caller's order) and the act_mask
 * bits moved with their segments (act_mask_out, may be NULL).  Callers see none of it: every output lands in its own segment's y. */
#define AMQ_GEMV_ROUTE_GENERIC 0
#define AMQ_GEMV_ROUTE_KEYED   1
int amq_gemv_route(int prologue, int M, int K, int group, int nseg, const int* bits /* host [nseg] */, const int* modes /* host [nseg] */,
                   const amq_gemv_opts* opts /* host, may be NULL */);
int amq_gemv_segment_order(int nseg, const int* bits /* host [nseg] */, int act_mask, int* order /* host [nseg], out */, int* act_mask_out);

/* kernel family of amq_gemm_route_f16 (AUTO = what every other GEMM entry point uses: chosen by shape) */
#define AMQ_GEMM_AUTO   0
#define AMQ_GEMM_TILED  1          /* LDS-DMA double-buffered 64/128-row tiles (+ split-K for few rows) */
#define AMQ_GEMM_SKINNY 2          /* barrier-free K-split-by-wave kernel, M <= 64 */
#define AMQ_GEMM_RING   3          /* 256 x 256 tiles (128 x 256 when those would not fill the chip), LDS rings for x and packed W, counted waits */
#define AMQ_GEMM_RING128 4         /* the same kernel forced to 128-row tiles */
#define AMQ_GEMM_WS 5              /* amq_gemm_ws.hip: 256 x 128 tiles, 4 MFMA waves + 4 DMA / unpack waves per workgroup (AUTO takes it where that tile fills the chip better) */
#define AMQ_GEMM_DEQ 6             /* dequantize once into the caller's workspace (N * K * 2 bytes), then amq_gemm_f16.hip: a plain fp16 GEMM with no
                                      unpack in its loop -- GPTQLinear.forward's own split from 128 rows on (hqq/backends/autogptq.py:245-283), hand-written.
                                      AUTO takes it for MFMA-bound launches when the workspace is passed. */

/* capabilities: writes up to `cap` ints {max GEMV rows for K (any options / group size), LDS limit, tile rows, tile columns, max GEMV rows for K
 * with default options over groups of 128, the same without an RMSNorm prologue (x may then be staged in two K phases)}; returns the count */
int amq_query(int K, int* out, int cap);

/* ---- native buffer sizes ------------------------------------------------ */
size_t amq_native_qweight_bytes(int bits, int N, int K);
float amq_fma1_scale_bound(int bits);   /* largest |scale| of an AMQ_MODE_FMA1 buffer: 65504 / 2^18 (4 bit), 65504 / 2^20 (2, 3 bit) */
size_t amq_native_meta_bytes(int N, int K, int group);

/* ---- load-time repack: reference formats -> native ---------------------- */
/* Format A: HQQLinear.W_q (uint8 for 4/2 bit, int32 for 3 bit) + meta['scale'], meta['zero'] fp16 [N*K/group]
 * (hqq/core/bitpack.py:24-110, quantize.py:106-111).  Result carries AMQ_MODE_HQQ. */
int amq_repack_from_hqq(int bits, const void* W_q, const void* scale, const void* zero,
                        int N, int K, int group, void* qweight_native, void* meta_native, void* stream);
/* Format B: GPTQLinear buffers qweight int32 [K/32*bits, N], scales fp32 [K/group, N], zeros fp32 [K/group, N]
 * (hqq/backends/autogptq.py:55-75).  Result carries AMQ_MODE_FMA (c = -zeros). */
int amq_repack_from_gptq(int bits, const void* qweight, const void* scales, const void* zeros,
                         int N, int K, int group, void* qweight_native, void* meta_native, void* stream);
/* Format C: FT_QuantLinear buffers qweight int16 [N/4, K], scales fp16 [K/group, N], scaled_zeros fp16
 * (hqq/backends/ft.py:57-126), 4 bit only.  Result carries AMQ_MODE_FMA (c = scaled_zeros). */
int amq_repack_from_awq(const void* qweight, const void* scales, const void* scaled_zeros,
                        int N, int K, int group, void* qweight_native, void* meta_native, void* stream);

/* ---- quantize: dense fp16 -> Format A -------------------------------------- */
/* Quantizer.quantize with its proximal solver (hqq/core/quantize.py:76-180, optimize.py:96-108, 201-255: axis 1, lp_norm 0.7, beta 10,
 * 20 iterations, early stop on the tensor's mean |W - W_r|) in the fp32 arithmetic of the reference's CPU path, as three launches on `stream`
 * (solve: one pass over W, all 20 iterations in registers; stop: the tensor-wide decision; emit: codes packed as Format A).  No host read, no
 * allocation, no atomics; the grid and every summation order depend on (N, K, group) only, so a layer quantizes to the same bits on every run.
 *   W          fp16 [N, K], 8-byte aligned
 *   W_q        Format A: uint8 [R * bits / 8, group] (4 / 2 bit) or int32 [ceil(R / 10), group] (3 bit), R = N * K / group
 *   scale/zero fp16 [R]: the dequant multiplier 1 / s and the zero, as HQQLinear.meta holds them
 *   info       AMQ_HQQ_INFO_BYTES: {int32 stop iteration, int32 nonfinite (!= 0: W held an inf or NaN, the outputs are meaningless),
 *              float mean_err[20]: the tensor's mean |W - W_r| at the start of every iteration}
 *   workspace  amq_hqq_quantize_workspace_bytes(N, K, group) = 4 * (21 * R + 21 * wgs) bytes, 4-byte aligned, where
 *              P = R (R / 2 for group 32), T = ceil(P / 4096), wgs = ceil(P / (4 * T)); 0 for a shape the call refuses
 *   round_zero 0 / 1: round the initial zero (the reference's default is bits == 4)
 * Refused, in this order: a null pointer or a misaligned W (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); group not 32 / 64 / 128 / 256,
 * N % 16, K % 128 or K % group (AMQ_ESHAPE); workspace_bytes too small (AMQ_EINVAL). */
#define AMQ_HQQ_INFO_BYTES 88
size_t amq_hqq_quantize_workspace_bytes(int N, int K, int group);
int amq_hqq_quantize_f16(const void* W, int N, int K, int bits, int group, int round_zero, void* W_q, void* scale, void* zero,
                         void* info, void* workspace, size_t workspace_bytes, void* stream);

/* GPTQ's error-feedback solve (asymmetric, grouped, no act-order, no static groups; blocks of 128 columns) to the same Format A, as three launches on
 * `stream` (solve, nonfinite flag, pack).  All fp32, every operation its own rounding, IEEE division, round-half-even.  Per row, columns ascending:
 * at the start of each 128-column block every group in it takes xmin = min(min(x), 0), xmax = max(max(x), 0) of the row's CURRENT values (-1 / +1 if
 * both are 0), s = (xmax - xmin) / maxq, s16 = max(fp16(s), 2^-24), z = rint(-xmin / s16); column i: q = clamp(rint(w / s16) + z, 0, maxq),
 * w^ = fp16((q - z) * s16) -- the weight amq_dequantize_hqq_f16 and the matmul kernels produce --, e = (w - w^) / U[i,i],
 * loss += ((w - w^)^2 / U[i,i]^2) / 2; then w_j -= e * U[i,j] (one multiply, one subtract) for every j > i, each element in ascending i.
 * No host read, no allocation, no atomics; rows are independent.
 *   W          fp16 [N, K], 16-byte aligned; the caller has zeroed the columns whose Hessian diagonal is 0
 *   U          fp32 [K, K], 16-byte aligned: the upper Cholesky factor of the damped inverse Hessian (only its upper triangle is used)
 *   W_q        Format A as above; scale = s16, zero = z (an integer), fp16 [R]
 *   row_loss   fp32 [N]
 *   info       AMQ_GPTQ_INFO_BYTES: {int32 nonfinite (!= 0: some w, e or U[i,i] was not finite, or U[i,i] <= 0: the outputs are meaningless)}
 *   workspace  amq_gptq_quantize_workspace_bytes(N, K, group) = 5 * N * K + N bytes (fp32 errors [N, K], int32 flags [N / 4], byte codes [N, K]),
 *              16-byte aligned; 0 for a shape the call refuses
 * Refused, in this order: a null or misaligned pointer (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); group not 32 / 64 / 128 (256 spans two
 * blocks), N % 16, K % 128 (AMQ_ESHAPE); workspace_bytes too small (AMQ_EINVAL). */
#define AMQ_GPTQ_INFO_BYTES 4
size_t amq_gptq_quantize_workspace_bytes(int N, int K, int group);
int amq_gptq_quantize_f16(const void* W, const void* U, int N, int K, int bits, int group, void* W_q, void* scale, void* zero, void* row_loss,
                          void* info, void* workspace, size_t workspace_bytes, void* stream);

/* The same solve with static groups and an activation order (gptq.py fasterquant(actorder=True, static_groups=True)), to the same Format A in W's
 * OWN column order, as four launches on `stream` (parameters, solve, nonfinite flag, pack).  First, for every row and every group of `group`
 * consecutive columns of W as handed in: xmin = min(min(x), 0), xmax = max(max(x), 0) (-1 / +1 if both are 0), s = (xmax - xmin) / maxq,
 * s16 = max(fp16(s), 2^-24), z = rint(-xmin / s16) -- the arithmetic above, applied once to the ORIGINAL values instead of per block to the
 * running ones.  Then per row the columns are walked in perm's order, i = 0 .. K - 1 ascending, in blocks of 128: walk column i is original column
 * perm[i], w its running value, (s16, z) those of group perm[i] / group; q = clamp(rint(w / s16) + z, 0, maxq), w^ = fp16((q - z) * s16),
 * e = (w - w^) / U_p[i,i], loss += ((w - w^)^2 / U_p[i,i]^2) / 2; then w_j -= e * U_p[i,j] (one multiply, one subtract) for every walk column
 * j > i, each element in ascending i.  The code of walk column i is column perm[i] of the packed layer: nothing at inference time knows the order.
 * All fp32, every operation its own rounding, IEEE division, round-half-even.  No host read, no allocation, no atomics; rows are independent.
 *   W          fp16 [N, K], 16-byte aligned, in its own column order; the caller has zeroed the columns whose Hessian diagonal is 0
 *   U_p        fp32 [K, K], 16-byte aligned: the upper Cholesky factor of the damped inverse of the PERMUTED Hessian H[perm][:, perm]
 *   perm       int32 [K], 16-byte aligned: a permutation of 0 .. K - 1.  The entry point cannot read it: the caller guarantees it (an entry
 *              outside 0 .. K - 1 is read as 0 and sets info; a repeated entry leaves codes unwritten).  The identity: static groups alone.
 *   W_q, scale, zero, row_loss, info   as for amq_gptq_quantize_f16
 *   workspace  amq_gptq_quantize_static_workspace_bytes(N, K, group) = 5 * N * K + N bytes (fp32 errors [N, K] in walk order, int32 flags [N / 4],
 *              byte codes [N, K] in W's order), 16-byte aligned; 0 for a shape the call refuses
 * Refused, in this order, as amq_gptq_quantize_f16: a null or misaligned pointer (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); group not
 * 32 / 64 / 128, N % 16, K % 128 (AMQ_ESHAPE); workspace_bytes too small (AMQ_EINVAL). */
size_t amq_gptq_quantize_static_workspace_bytes(int N, int K, int group);
int amq_gptq_quantize_static_f16(const void* W, const void* U_p, const void* perm, int N, int K, int bits, int group, void* W_q, void* scale,
                                 void* zero, void* row_loss, void* info, void* workspace, size_t workspace_bytes, void* stream);

/* AWQ's weight-side passes (awq_utils/quantizer.py pseudo_quantize_tensor with zero_point, auto_clip.py auto_clip_layer_asym) to the same Format A.
 * All fp32, every operation its own IEEE rounding, IEEE division, rint = round-half-even, no contraction except the fmaf written out below.
 * RTN of one group v[0..G) of fp16 values: maxq = 2^bits - 1, xmax = max v, xmin = min v, s = max(xmax - xmin, 1e-5f) / maxq, s16 = fp16(s) (never
 * 0: s >= 1e-5 / 15 > 2^-24), z = clamp(rint(-xmin / s16), 0, maxq) + 0 (a -0 becomes +0), q = clamp(rint(v / s16) + z, 0, maxq), w^ = fp16((q - z) * s16) -- the weight
 * amq_dequantize_hqq_f16 and the matmul kernels produce from scale = s16, zero = z.  (Unlike the GPTQ rule, 0 is not forced into the range and z is
 * clamped, as AWQ does; the scale is rounded to fp16 BEFORE it is used, the deployment deviation of the GPTQ solve.)
 *
 * amq_awq_quantize_f16: v = col_scale ? fp16(fp32(w) * c_k) : w; with bounds v = min(max(v, lo), hi) of the element's group; RTN per group.
 *   W          fp16 [N, K], 16-byte aligned
 *   col_scale  fp32 [K] or NULL
 *   hi, lo     fp16 [N, K / group], both or neither
 *   W_q, scale, zero   Format A as above (scale = s16, zero = z), all three or none
 *   dense      fp16 [N, K] or NULL: col_scale ? fp16(fp32(w^) / c_k) : w^ (the scale search's w_quantize_func(W s) / s); 16-byte aligned
 *   info       AMQ_AWQ_INFO_BYTES: {int32 nonfinite (!= 0: a scaled weight, a bound or a dense output was not finite: the outputs are meaningless)}
 *   workspace  amq_awq_quantize_workspace_bytes(N, K, group) = N * K / 128 + N * K bytes (int32 flags [N * K / 512], byte codes [N, K]), 16-byte
 *              aligned; 0 for a shape the call refuses
 * Three launches (round, nonfinite flag, pack; two without Format A).  No host read, no allocation, no atomics: the same bits on every run.
 *
 * amq_awq_clip_f16: W fp16 [N, K] (the layer's current, already column-scaled weights), X fp16 [T, K] (the sampled activation rows).  For every
 * row n, group g and step i = 0..9: f_i = the fp32 nearest to 1 - i / 20; hi_i = fp16(fp32(max_g) * f_i), lo_i = fp16(fp32(min_g) * f_i); w^_i =
 * RTN of the group clamped to [lo_i, hi_i] with the clamped group's own min and max; d_i[c] = fp32(w^_i[c]) - fp32(w[c]); o_i[t] = the chain
 * acc = fmaf(fp32(x[t, c]), d_i[c], acc) over the group's columns in ascending c from acc = 0; err_i = the sum of o_i[t] * o_i[t] (one multiply per
 * term) in THIS order: with t = 16 a + 4 h + r (h, r in 0..3; rows t >= T are zeros and add exactly 0), P_h = the running sum from 0 over a
 * ascending, r ascending inside a; err_i = (P_0 + P_1) + (P_2 + P_3).  The order depends on T only.  The winner is the lowest i with the smallest
 * err_i (strict <: the least shrink wins a tie; step 0 is plain RTN).
 *   hi, lo     fp16 [N, K / group]: the winner's bounds
 *   best       int32 [N, K / group]: the winner's step
 *   err        fp32 [N, K / group, 10]: the sums (not divided by T)
 *   info       AMQ_AWQ_INFO_BYTES: {int32 nonfinite (!= 0: a weight or a sum was not finite)}
 *   workspace  amq_awq_clip_workspace_bytes(N, K, T, group) = 4 * (N / 8) * (K / group) bytes, 4-byte aligned; 0 for a shape the call refuses
 * One wave per (8 rows, group): the chains run on v_mfma_f32_16x16x4_f32, which is bit for bit that fmaf chain.  Two launches (search, flag).
 *
 * Refused, in this order: a null or misaligned pointer (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); group not 32 / 64 / 128, N % 16, K % 128,
 * T < 1 (AMQ_ESHAPE); workspace_bytes too small (AMQ_EINVAL). */
#define AMQ_AWQ_INFO_BYTES 4
size_t amq_awq_quantize_workspace_bytes(int N, int K, int group);
int amq_awq_quantize_f16(const void* W, const void* col_scale, const void* hi, const void* lo, int N, int K, int bits, int group, void* W_q,
                         void* scale, void* zero, void* dense, void* info, void* workspace, size_t workspace_bytes, void* stream);
size_t amq_awq_clip_workspace_bytes(int N, int K, int T, int group);
int amq_awq_clip_f16(const void* W, const void* X, int N, int K, int T, int bits, int group, void* hi, void* lo, void* best, void* err,
                     void* info, void* workspace, size_t workspace_bytes, void* stream);

/* OWQ (amq/quantization/owq.py: OWQ.run, GPTQ_OWQ, Quantizer.find_params with mse, asymmetric, per channel): n_out input columns of a linear stay
 * fp16 and absorb the error feedback of the quantized ones; every 128-column group of the rest takes its range from a candidate search.  Groups
 * of 128 only.  All fp32, every operation its own IEEE rounding, IEEE division, rint = round-half-even, except the score's power below.
 *
 * Range search of a segment v[0..L) with maxq = 2^bits - 1: xmin = min(min v, 0), xmax = max(max v, 0), xrange = xmax - xmin; for i = 1..num:
 * tmp_max = (xrange / num) * i, delta = max(tmp_max / maxq, 1e-8f), d16 = max(fp16(delta), 2^-24), r_c = rint(v_c / d16); for zp = 0..maxq:
 * q_c = clamp(r_c + zp, 0, maxq), w^_c = fp16((q_c - zp) * d16) -- the weight amq_dequantize_hqq_f16 produces from scale d16 and zero zp --,
 * score = (sum_c |v_c - w^_c|^2.4) / L.  The winner is the first candidate in (i ascending, zp ascending) order with the strictly smallest score,
 * starting from 1e10; the result is (scale = d16, zero = zp, i, zp, score) of the winner.  |d|^2.4 is exp2(2.4f * log2(d)) on the hardware's
 * v_log_f32 / v_exp_f32 (1 ulp each; 0 and denormal d give 0): the one place where bits may differ from a host restatement.  A row that holds a
 * non-finite value ends without a winner (i = 0, scale = 0, score = 1e10).
 *
 * amq_owq_range_f16: the search of W[n, col0 .. col0 + L) for every row n, one workgroup of 256 threads per row, the segment staged in LDS.
 * The sum's order: thread t adds its elements c = t, t + 256, ... in ascending c from 0; a wave's 64 sums meet in a butterfly (xor 1, 2, 4, 8, 16,
 * 32); the four waves' sums are (w0 + w1) + (w2 + w3).
 *   W          fp16 [N, K]
 *   scale/zero fp16 [N]; choice int32 [N, 2] = (i, zp); score fp32 [N]
 *   wq_err     fp32 [K] or NULL; only with col0 = 0, L = K: frob_c = the sum over the rows n ascending (one chain) of (w - w^)^2, one multiply and
 *              one add per row, w^ the row's deployed weight under its winner
 *   info       AMQ_OWQ_INFO_BYTES: {int32 nonfinite (!= 0: some row ended without a winner)}
 * Refused, in this order: a null or misaligned pointer (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); N % 16, K % 128, num outside 1..100, a
 * segment outside the row or longer than 30720 (LDS), wq_err without the whole row (AMQ_ESHAPE).  Up to three launches (search, column sums, flag).
 *
 * amq_owq_quantize_f16: the solve over the PERMUTED W_p [N, K] (the n_out outlier columns last) and U_p = the upper Cholesky factor of the damped
 * inverse of the equally permuted Hessian; the caller has zeroed dead columns.  n_nonout = K - n_out.  Per row, columns ascending, blocks of 128,
 * as amq_gptq_quantize_f16 above with three differences: (a) at a block's start its group takes (d16, zp) from the range search over the row's
 * CURRENT values of the group's columns < n_nonout (the last group may be ragged, L = n_nonout mod 128; the sum's order: a lane adds its up to 8
 * consecutive columns ascending from 0, the row's 16 lanes meet in a butterfly, xor 1, 2, 4, 8); (b) columns >= n_nonout are never quantized and
 * contribute no error: they receive w_j -= e * U[i,j] of every earlier quantized column i, each element in ascending i, and leave as
 * W_out = fp16(w_j); (c) the packed result has Kp = 128 * ceil(n_nonout / 128) columns and the padding columns of a ragged last group take the
 * code zp, so they dequantize to exactly 0.  n_out = 0 is GPTQ with searched ranges.
 *   W_p        fp16 [N, K], U_p fp32 [K, K], both 16-byte aligned
 *   W_q        Format A of a layer [N, Kp] in groups of 128; scale = d16, zero = zp, fp16 [N * Kp / 128]
 *   W_out      fp16 [N, n_out] (may be NULL when n_out = 0): the outlier columns in W_p's order
 *   choice     int32 [N, Kp / 128, 2]: the winner's (i, zp) per row and group
 *   row_loss   fp32 [N]: the quantized columns' ((w - w^)^2 / U[i,i]^2) / 2, summed in ascending i
 *   info       AMQ_OWQ_INFO_BYTES: {int32 nonfinite (!= 0: some w, e or U[i,i] was not finite, U[i,i] <= 0 or a group had no winner)}
 *   workspace  amq_owq_quantize_workspace_bytes(N, K, n_out, group) = 5 * N * Kp + N bytes (fp32 errors [N, Kp], int32 flags [N / 4], byte codes
 *              [N, Kp]), 16-byte aligned; 0 for a shape the call refuses
 * Refused, in this order: a null or misaligned pointer (AMQ_EINVAL); bits not 2 / 3 / 4 (AMQ_EINVAL); group not 128, N % 16, K % 128, num outside
 * 1..100, n_out odd, negative or >= K (AMQ_ESHAPE); workspace_bytes too small (AMQ_EINVAL).  Three launches (solve, nonfinite flag, pack).
 *
 * The deployment side of a layer y = xg . Wq^T + x[:, out_ids] . W_out^T (two entry points around the packed matmul):
 * amq_owq_gather_f16: xg[m, c] = x[m, perm[c]], and 0 where perm[c] is not in 0 .. K - 1 (the padding columns: a 0 weight must not meet an inf).
 *   x fp16 [M, K], perm int32 [Kp], xg fp16 [M, Kp], Kp % 128 == 0
 * amq_owq_outlier_add_f16: after the packed matmul over xg has written y, y[m, n] = fp16(fp32(y[m, n]) + acc), acc = the fmaf chain over j ascending
 * of fp32(x[m, out_ids[j]]) * fp32(W_out[n, j]) from 0.
 *   out_ids int32 [n_out] ascending, W_out fp16 [N, n_out] with its columns in that order, y fp16 [M, N], M <= 65535
 * None of these calls reads on the host, allocates or uses atomics: the same bits on every run, capturable. */
#define AMQ_OWQ_INFO_BYTES 4
int amq_owq_range_f16(const void* W, int N, int K, int col0, int L, int bits, int num, void* scale, void* zero, void* choice, void* score,
                      void* wq_err, void* info, void* stream);
size_t amq_owq_quantize_workspace_bytes(int N, int K, int n_out, int group);
int amq_owq_quantize_f16(const void* W_p, const void* U_p, int N, int K, int n_out, int bits, int group, int num, void* W_q, void* scale,
                         void* zero, void* W_out, void* choice, void* row_loss, void* info, void* workspace, size_t workspace_bytes,
                         void* stream);
int amq_owq_gather_f16(const void* x, int M, int K, const void* perm, int Kp, void* xg, void* stream);
int amq_owq_outlier_add_f16(const void* x, int M, int K, const void* out_ids, int n_out, const void* W_out, void* y, int N, void* stream);

/* amq_owq_stage_f16: the token step's stage of OWQ layers -- ONE launch in front of the unchanged packed GEMVs of up to three sibling linears that
 * read the same activation a of R = 1 .. 8 rows of x [R, K]:
 *   AMQ_OWQ_ACT_NONE      a = x
 *   AMQ_OWQ_ACT_RMSNORM   a = what amq_rmsnorm_f16(x, gamma, eps) writes (the statistic in its kernel's order:
 *                         thread t of 256 adds the squares of the 8-element chunks t, t + 256, ..., a wave's sums meet in the xor
 *                         32, 16, .. 1 butterfly, the four waves' sums are added in order); every workgroup takes it for itself
 *   AMQ_OWQ_ACT_SILU_MUL  a = what amq_silu_mul_f16(x, x2) writes, x2 [R, K]
 * and per part (host structs, as amq_segment):
 *   xg[r, c] = a[r, perm[c]], 0 where perm[c] is not in 0 .. K - 1                                         (amq_owq_gather_f16 over a)
 *   y[r, n]  = fp16(acc), or fp16(fp32(residual[r, n]) + acc) with a residual (which may be y itself); acc = the fmaf chain over j ascending of
 *              fp32(a[r, out_ids[j]]) * fp32(W_out[n, j]) from 0                                           (amq_owq_outlier_add_f16 over a)
 * so that amq_gemv_grouped_f16(xg, segment {y, residual = y}) completes the layer.  A part with n_out == 0 is a plain sibling: perm, out_ids, W_out,
 * y, residual, N and Kp are not looked at, and xg [R, K] receives a itself.  The results are bit for bit those of the entry points named above in
 * composition.  One launch; no host read, no allocation, no atomics: the same bits on every run, capturable.
 * Refused, in this order: x, parts, gamma (RMSNORM) or x2 (SILU_MUL) null, or x / x2 / gamma not 16-byte aligned (AMQ_EINVAL); an unknown act
 * (AMQ_EINVAL); n_parts outside 1 .. 3, R outside 1 .. 8, K % 128 (AMQ_ESHAPE); then part by part: a null xg, or with outliers a null perm, out_ids,
 * W_out or y, or a misaligned pointer -- xg and perm / out_ids 4-byte, the rest 2-byte -- (AMQ_EINVAL); n_out negative, odd or >= K, Kp % 128 or
 * Kp <= 0, N <= 0 (AMQ_ESHAPE). */
#define AMQ_OWQ_ACT_NONE     0
#define AMQ_OWQ_ACT_RMSNORM  1
#define AMQ_OWQ_ACT_SILU_MUL 2
#define AMQ_OWQ_MAX_PARTS    3
typedef struct amq_owq_part {
    const void* perm;      /* int32 [Kp]: the packed layer's columns in x's numbering, -1 = padding */
    const void* out_ids;   /* int32 [n_out] */
    const void* W_out;     /* fp16 [N, n_out] */
    void* xg;              /* fp16 [R, Kp] (n_out == 0: [R, K]) */
    void* y;               /* fp16 [R, N] */
    const void* residual;  /* fp16 [R, N] or NULL; may be y */
    int N, n_out, Kp;
} amq_owq_part;
int amq_owq_stage_f16(const void* x, int R, int K, int act, const void* gamma, float eps, const void* x2, const amq_owq_part* parts, int n_parts,
                      void* stream);

/* ---- dequantize ---------------------------------------------------------- */
/* native -> W[N,K] fp16 (row-major, nn.Linear orientation) */
int amq_dequantize_f16(int bits, int mode, const void* qweight_native, const void* meta_native,
                       int N, int K, int group, void* W_out, void* stream);
/* Format A -> W[N,K] fp16: Quantizer.dequantize (quantize.py:184-199) as one kernel */
int amq_dequantize_hqq_f16(int bits, const void* W_q, const void* scale, const void* zero,
                           int N, int K, int group, void* W_out, void* stream);

/* ---- the hot path: y[M,N] = x[M,K] . W^T (+ bias) ------------------------ */
/* few rows (decode).  The unpacked weights are the MFMA B operand straight from registers (W never touches LDS); the x rows are staged in LDS.
 * M <= 16 and the rows must fit LDS: M * (K + 8) * 2 bytes + the cross-wave sum buffer (4 - 32 KiB by row count) <= 160 KiB -- except that with
 * default options, no RMSNorm prologue and 5 .. 8 rows a K whose rows do not fit whole is staged in two K phases (8 rows of K = 11008).
 * amq_query(K) returns the row limits; AMQ_ESHAPE beyond -- use amq_gemm_f16.  x_stride / y_stride in elements (0 = dense; 2 .. 8 dense rows
 * take the LDS-DMA staging path, strided rows the generic one: same results).
 *
 * ROW STRIDES of every fp16 matmul entry point of this header (x_stride, y_stride, amq_segment.y_stride), checked on the host before anything is
 * launched, AMQ_ESHAPE otherwise: a stride is 0 (dense) or at least the row it steps over (x_stride >= K, y_stride >= N; never negative);
 * x_stride % 8 == 0 (rows of x are read in 16-byte pieces) and y_stride % 8 == 0 (the split-K reduce accesses y and the residual in 16-byte pieces;
 * one rule for every entry point; amq_gemm_f16w_f16 alone asks y_stride % 4 == 0 only).  The residual is read with y's stride.  Where the few-row
 * GEMM kernel can serve the call (M <= 256; routes AMQ_GEMM_AUTO and _SKINNY), strided rows of x must span fewer than 2^31
 * elements.  Dense calls meet all of it by N % 16 == 0,
 * K % 128 == 0.  Nothing outside the N columns of a row of y is written, and nothing outside the K columns of a row of x is read. */
int amq_gemv_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                 const void* bias, void* y, int M, int N, int K, int group,
                 int x_stride, int y_stride, void* stream);
/* any M (prefill / batched): LDS-staged x tiles, MFMA 16x16x32 f16.  x_stride / y_stride: the row-stride rule above (0, or >= K / N and % 8 == 0) */
int amq_gemm_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                 const void* bias, void* y, int M, int N, int K, int group,
                 int x_stride, int y_stride, void* stream);
/* dispatch the way the reference modules do (rows < threshold -> gemv, else gemm;
 * GPTQLinear.forward autogptq.py:163, FT_QuantLinear.forward_normal ft.py:128-145) */
int amq_linear_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                   const void* bias, void* y, int M, int N, int K, int group, void* stream);

/* Few-row GEMM (16 < M <= ~256: short prompts) with split-K: a launch whose M x N tiles would occupy fewer than 192
 * workgroups splits the K loop over up to 8 workgroup layers; each layer writes fp32 partials into its own slice of a
 * caller-owned workspace, a second kernel sums the slices in a fixed order (deterministic, no atomics).
 * amq_gemm_splitk_workspace_bytes() returns the bytes required (0: the shape does not split and no workspace is
 * needed; the call then forwards to amq_gemm_f16).  x_stride / y_stride: the row-stride rule above (0, or >= K / N and % 8 == 0).  Replaces the reference's cross-CTA split-K of gemm_w4a16_T1
 * (amq/kernel/ft/quantization_new/gemm/gemm_cuda.cu:514-584: semaphore + __hadd2 read-modify-write of C). */
size_t amq_gemm_splitk_workspace_bytes(int M, int N, int K);
int amq_gemm_splitk_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                        const void* bias, void* y, int M, int N, int K, int group, int x_stride, int y_stride,
                        void* workspace, size_t workspace_bytes, void* stream);

/* several linears that consume the same x (q/k/v, gate/up), each with its own bit-width,
 * in ONE launch; optional fused prologue on x and residual add on y.  x_stride (0 = K; else >= K and % 8 == 0) is the row stride of x AND of x2:
 * the second operand of AMQ_PRO_SILU_MUL / AMQ_PRO_MUL is read at x2 + row * x_stride. */
typedef struct amq_segment {
    const void* qweight_native;
    const void* meta_native;
    const void* bias;       /* fp16 [N] or NULL */
    const void* residual;   /* fp16 [M, y_stride] or NULL: y = residual + (x W^T + bias) */
    void* y;                /* fp16 [M, y_stride] */
    int N;
    int bits;
    int mode;
    int y_stride;           /* 0 = N; else >= N and % 8 == 0 (the row-stride rule above); several segments may share one [M, y_stride] buffer, each at
                             * its own column offset (fused q/k/v): a segment writes its N columns of a row and nothing else */
} amq_segment;

int amq_gemv_grouped_f16(const amq_segment* segments /* host */, int nseg,
                         const void* x, const void* x2, const void* gamma, float eps, int prologue,
                         int M, int K, int group, int x_stride, const amq_gemv_opts* opts /* host, may be NULL */,
                         void* stream);
/* 2 .. 8 rows (sequences decoded together), RMSNorm WITHOUT a pass over x for its statistic: a launch that writes a hidden state (o_proj, down_proj:
 * ONE segment, residual in the epilogue) also leaves, per row, one sum of squares per 16 output columns in sums_out (fp32 [M][N / 16], written
 * whole by every launch); the launch that normalises that hidden state takes them as sums_in (fp32 [M][K / 16]) with gamma and eps, adds them
 * in a fixed order and only applies gamma * fp16(x * rstd) while staging x -- LlamaRMSNorm's value up to the summation order of its fp32
 * mean (the fused AMQ_PRO_RMSNORM prologue repeats the whole statistic in every workgroup -- ~90 VALU instructions per row and thread: at 5 .. 8
 * rows that costs more than a separate amq_rmsnorm_f16 launch; this form costs less than either, from 2 rows on).  sums_in == NULL: no prologue (then gamma must be NULL too); sums_out == NULL: none
 * written.  x dense [M][K], groups of 128, default arithmetic; K <= 8192 with sums_in.  Replaces layernorm.cu:25-51 + the GEMV behind it in the
 * reference's FT step (ftllama_modeling.py:39-46) for Batch 2 .. 8 (gemv_cuda.cu:381-437 makes batches first-class). */
int amq_gemv_grouped_sums_f16(const amq_segment* segs, int nseg, const void* x, const void* gamma, float eps, const float* sums_in,
                              float* sums_out, int M, int K, int group, void* stream);


/* ---- entry points shaped like the reference's pybind functions ------------------------------------
 * They take the reference's own buffers (Format B / Format C) unchanged.  The HIP kernels read the native layout,
 * so each call needs a caller-owned `workspace` of at least amq_compat_workspace_bytes(bits, M, N, K) bytes; the
 * native copy of the weights is (re)built into it unless `workspace_valid` != 0 (pass 0 on the first call for a given
 * weight, 1 afterwards: the repack is then skipped and the call costs the same as amq_linear_f16).
 *
 * amq_vecquantmatmul_faster_old  <->  auto_gptq.vecquant{2,3,4}matmul_faster_old(vec, mat, mul, scales, zeros,
 *     groupsize, vec_height)                (auto_gptq_kernel.cu:129-158, 227-256, 345-374, 443-467)
 *     vec fp16 [batch, K], mat int32 [K/32*bits, N], mul fp32 [batch, N] ACCUMULATED IN PLACE (mul += vec . W),
 *     scales / zeros fp32 [K/groupsize, N]; height = mat rows, width = N; vec_height (= K/2) is accepted and checked.
 * amq_gemv_4bit  <->  faster_transformer.gemv_4bit(x, kernel, scales, scaled_zeros, m, n, k, group_size) -> y
 *     (gemv_cuda.cu:358-437); the reference throws for m outside 1..7, here any m >= 1 works.
 * amq_gemm_4bit  <->  faster_transformer.gemm_4bit(x, kernel, scales, scaled_zeros) -> y   (gemm_cuda.cu:929-1033)
 *     x fp16 [m, k], kernel int16 [n/4, k], scales / scaled_zeros fp16 [k/group, n], y fp16 [m, n] (caller-allocated). */
size_t amq_compat_workspace_bytes(int bits, int M, int N, int K);
int amq_vecquantmatmul_faster_old(int bits, const void* vec, const void* mat, void* mul, const void* scales,
                                  const void* zeros, int groupsize, int vec_height, int batch, int height, int width,
                                  void* workspace, size_t workspace_bytes, int workspace_valid, void* stream);
int amq_gemv_4bit(const void* x, const void* kernel, const void* scales, const void* scaled_zeros, void* y,
                  int m, int n, int k, int group_size,
                  void* workspace, size_t workspace_bytes, int workspace_valid, void* stream);
int amq_gemm_4bit(const void* x, const void* kernel, const void* scales, const void* scaled_zeros, void* y,
                  int m, int n, int k, int group_size,
                  void* workspace, size_t workspace_bytes, int workspace_valid, void* stream);

/* ---- decode-step surroundings (next tier: what sits between the linears in one token step) ---- */
/* y = gamma * fp16(x * rsqrt(mean(x^2) + eps)), rows of K; replaces FT layernorm_forward_cuda (ft/layernorm/layernorm.cu:25-77) */
int amq_rmsnorm_f16(const void* x, const void* gamma, void* y, int M, int K, float eps, void* stream);
/* y[N] = (optionally RMSNorm'ed) x[K] . W^T for fp16 W[N,K] (lm_head), K % 8 == 0; gamma NULL = no norm */
int amq_gemv_f16w(const void* x, const void* W, const void* bias, void* y, const void* gamma, float eps,
                  int N, int K, void* stream);
/* the same for M = 1 .. 8 rows (batched decode): x fp16 [M, K], y fp16 [M, N], both contiguous; W is streamed once */
int amq_gemv_f16w_rows(const void* x, const void* W, const void* bias, void* y, const void* gamma, float eps, int M,
                       int N, int K, void* stream);
/* ---- the 8-bit lm_head, "LM8" (additive, AMQ_VERSION unchanged) ----
 * codes uint8 [N, K] row-major; meta fp16 [N, K / 128, 2] = (scale, zero) of every group of 128 along K (HQQ conventions: the stored scale
 * multiplies, the zero is fractional).  The weight of a code c is w = fp16(fp16(fp16(c) - zero) * scale): two fp16 roundings, bit for bit the
 * reference's dequantize(), overflow to inf included.  group must be 128 and K a multiple of it.
 * amq_lm8_gemv_f16: y [M, N] = fp16 of the fp32 sum of exact fp16 products of x [M, K] (with gamma: gamma * fp16(x * rsqrt(mean x^2 + eps)), the
 * prologue of amq_gemv_f16w) with those weights; x and y contiguous, 1 <= M <= 8, W streamed once; the rows of an M-row call equal M one-row
 * calls bit for bit.  M rows of K rounded up to 1024 must fit LDS (AMQ_ESHAPE otherwise).
 * amq_lm8_dequantize_f16: rows row0 .. row0 + rows - 1 of the weights as fp16 [rows, K].
 * x, gamma, codes and out must be 16-byte aligned, meta 4-byte (AMQ_EINVAL otherwise). */
int amq_lm8_gemv_f16(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K, int group,
                     void* stream);
int amq_lm8_dequantize_f16(const void* codes, const void* meta, void* out, int row0, int rows, int N, int K, int group, void* stream);
/* one new token per sequence: RoPE(q, k) at position *pos_dev (or pos if pos_dev is NULL), append k/v to the
 * cache [B, n_kv_heads, max_seq, 128], out = softmax(q K^T / sqrt(128)) V.  head_dim must be 128.
 * Replaces FT single_query_attention (ft/attention/decoder_masked_multihead_attention.cu:30-61) with HF-Llama numerics. */
int amq_attn_decode_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                        const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                        int max_seq, float rope_theta, const void* rope_table, void* stream);
/* optional: fp16 [max_seq][64][2] (cos, sin) table for amq_attn_decode_f16 (NULL there = computed in-kernel, same values) */
int amq_rope_table_f16(void* table, int max_seq, float rope_theta, void* stream);
/* the same table from explicit inverse frequencies: inv_freq fp32 [64] on the device -- what HF's rotary embedding holds after a static
 * rope_scaling (Llama-3.1's "llama3" factors, "linear", ...; amq/configs/llama.json:82+ lists the Llama-3.x models) -- and its attention_scaling
 * factor (1 for those): table[pos][i] = (fp16(cos(pos * inv_freq[i]) * scale), fp16(sin(...) * scale)), LlamaRotaryEmbedding.forward's expression.
 * Every kernel that rotates (amq_attn_decode_*_f16 through the step-state row, amq_rope_cache_*, amq_rope_rows_f16) reads the table it is given. */
int amq_rope_table_freqs_f16(void* table, int max_seq, const float* inv_freq, float scale, void* stream);

/* Decode attention for graph-replayed token steps.  step_state is a 264-byte device block
 *     { fp16 cos/sin [64][2] of the CURRENT position ; int32 position at byte 256 ; int32 sticky error word at byte 260 }
 * that amq_decode_tail_f16 keeps up to date (pass rope_cur = step_state, pos = step_state + 256 there): position and
 * rotation inputs are fetched by the kernel's first instructions instead of through the position -> table-row chain of
 * dependent loads of amq_attn_decode_f16.
 * Both attention entry points treat a device-side position outside 0 .. max_seq-1 as a no-op (no cache append, no
 * output); this one also sets the error word to 1 (it is never cleared by the library: zero it when the state is
 * created, read it back to learn that a replay ran past the cache).  amq_decode_tail_f16 saturates the position at
 * rope_rows (= max_seq), so a runaway replay keeps hitting the no-op path. */
int amq_attn_decode_cur_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                            const void* step_state, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                            void* stream);

/* The same attention step for LONG contexts: n_splits workgroups share a head (grid = heads x batch x n_splits); the context
 * 0 .. pos is cut into at most n_splits chunks of >= 256 keys, each workgroup computes its chunk's scores, softmax statistics
 * and un-normalised output, leaves them in `workspace`, takes a ticket, and the last one to arrive (nobody waits) combines
 * them in chunk order.  amq_attn_decode_f16 walks a head's whole context on one CU -- right for a few hundred keys, 4.2 ms of
 * a 5.4 ms 7B token at 4000.  While the context fits ONE chunk (pos < 256, or n_splits == 1) the result is that of
 * amq_attn_decode_f16 / _cur_f16 bit for bit; with several chunks the probabilities are not rounded to fp16 before P.V
 * (exact softmax; within output rounding of the one-chunk result).  n_splits = ceil(max_seq / 384) keeps every chunk on the
 * kernel's register-prefetch path.  step_state != NULL: position / rotation from the step-state block (as _cur_f16; pos_dev,
 * pos, rope_theta, rope_table ignored); else as amq_attn_decode_f16.  workspace: amq_attn_decode_split_workspace_bytes bytes,
 * no initialisation; tickets: int32 [batch * n_heads], ZERO before the first launch, left zero by every launch; neither may
 * be shared by launches that can run concurrently.  The out-of-range position guard is the same (no-op, error word).
 * Grouped-query models (2 .. 16 query heads per kv head, n_splits > 1): ONE workgroup per (kv head, chunk) takes the chunk in once and scores it
 * against all the group's heads on the matrix cores, chunks of 128 * ceil(ceil(max_seq / n_splits) / 128) keys walked in double-buffered stages,
 * and a second small launch adds the chunks' partial results in chunk order (same workspace; the tickets are not used).  Its arithmetic is the
 * prompt kernel's (amq_attn_prefill_f16: fp32 scores, un-normalised probabilities rounded to fp16 before P.V) -- within fp16 output rounding
 * of the per-head kernels, also with one active chunk; deterministic.  Llama-3.1-8B heads at 8192 / 32768 cached keys: 23.6 -> 15.3 us,
 * 61 -> 33 us per launch (4.1 TB/s of K + V). */
size_t amq_attn_decode_split_workspace_bytes(int batch, int n_heads, int n_splits);
int amq_attn_decode_split_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                              const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads,
                              int head_dim, int max_seq, float rope_theta, const void* rope_table, int n_splits,
                              void* workspace, size_t workspace_bytes, void* tickets, void* stream);

/* 8-bit KV cache.  Per block four caller-owned tensors: kc8 / vc8 int8 [batch][n_kv_heads][max_seq][128] and ks / vs fp32
 * [batch][n_kv_heads][max_seq] -- one scale per (sequence, kv head, position), K and V separately; 132 bytes per row instead of 256.  A row r
 * (the fp16 values the fp16 cache would hold) is stored as a = max |r_i| (fp32), s = a / 127, c_i = clamp(rint(r_i / s), -127, 127) with ties to
 * even -- every step ONE rounded fp32 operation; a == 0 gives s = 0 and codes 0; a row that holds inf or NaN gives a NaN scale and codes 0.
 * The value a row stands for is fp32(c_i) * s.
 * amq_kv8_store_f16: the prompt pass.  k / v fp16 [batch * S][n_kv_heads * 128] contiguous (k ROTATED, e.g. by amq_rope_rows_f16) go into rows
 * pos0 .. pos0 + S - 1 of every sequence's slice in one launch. */
int amq_kv8_store_f16(const void* k, const void* v, void* kc8, void* ks, void* vc8, void* vs, int pos0, int S, int batch, int n_kv_heads,
                      int head_dim, int max_seq, void* stream);
/* amq_attn_decode_kv8_f16: one new token per sequence at a position shared by the batch.  q and the new k are rotated with the fp16 expression
 * of amq_attn_decode_f16, the new k / v rows are quantized (the bytes amq_kv8_store_f16 writes for the same row) and appended by exactly one
 * workgroup per (sequence, kv head), and out = softmax(q K^T / sqrt 128) V over the DEQUANTIZED rows 0 .. pos -- the new row included in its
 * dequantized form.  Scores (sum_i q_i c_ti) * s_t * (1 / sqrt 128) in fp32 (never rounded to fp16), softmax in fp32, probabilities NOT rounded
 * to fp16, sum_t (p_t s_t) c_ti in fp32, fp16 output.  1 .. 16 query heads per kv head: one workgroup serves up to 8 heads of a kv head from one
 * read of its rows.  n_splits >= 1 workgroups share a (sequence, kv head): chunks of ceil(max_seq / n_splits) keys rounded up to 32; chunks beyond
 * the position leave at once, the last arriver combines in chunk order (deterministic).  step_state != NULL: position / rotation / error word
 * from the step-state block (as amq_attn_decode_cur_f16; pos_dev, pos, rope_theta, rope_table ignored); else as amq_attn_decode_f16.  A device
 * position outside 0 .. max_seq - 1 is a no-op (nothing appended, no output; error word raised in step-state mode).  workspace:
 * amq_attn_decode_kv8_workspace_bytes bytes, no initialisation; tickets: int32 [batch * n_kv_heads * 2], ZERO before the first launch, left zero
 * by every launch; neither may be shared by launches that can run concurrently. */
size_t amq_attn_decode_kv8_workspace_bytes(int batch, int n_heads, int n_splits);
int amq_attn_decode_kv8_f16(const void* q, const void* k, const void* v, void* kc8, void* ks, void* vc8, void* vs, void* out,
                            const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                            int max_seq, float rope_theta, const void* rope_table, int n_splits, void* workspace, size_t workspace_bytes,
                            void* tickets, void* stream);

/* End of a greedy token step in one launch: token[0] = argmax(logits[0..vocab)) (first maximum), pos[0] += 1,
 * x[0..hidden) = embed[token][0..hidden); when rope_table / rope_cur are given (both or neither) also
 * rope_cur[0..128) = rope_table[min(pos, rope_rows - 1)][0..128), the cos/sin row amq_attn_decode_cur_f16 reads in the next step.  Replaces the `torch.argmax` / position increment / embedding gather that follow
 * the lm_head in the reference's generation loop (amq/utils/speed.py:70-76, HF `_sample`) when the step is replayed from
 * a hipGraph.  logits, embed, x: fp16; token: int64; pos: int32; all device pointers. */
int amq_decode_tail_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                        const void* rope_table, void* rope_cur, int rope_rows, void* stream);
/* Batched decode (several sequences at the SAME position, one step state): logits fp16 [batch, vocab], token int64 [batch],
 * x fp16 [batch, hidden]; pos / rope_cur are advanced once. */
/* The same with up to 8 token ids that are never chosen: suppress_ids = device int32 [8], -1 = unused slot (the values may change between replays
 * of a captured step; the pointer may not).  What HF's MinNewTokensLengthLogitsProcessor does to the EOS ids while min_new_tokens has not been
 * reached -- generate(min_new_tokens = max_new_tokens = n), amq/utils/speed.py:31-36 -- i.e. on every step of the reference's TPS loop. */
/* "This is the next input token" for a captured token step whose caller feeds the tokens itself (model(ids, start_pos=...) token by token,
 * amq/utils/speed.py:76-90): token[b] = token_in[b] (n_in == batch) or token_in[0] (n_in == 1), clamped to the vocabulary; x[b] = embed[token[b]];
 * rope_cur = rope_table[min(*pos, rope_rows - 1)] (both or neither, as above).  The position is not changed.  All pointers device. */
int amq_set_token_f16(const long long* token_in, int n_in, const void* embed, int vocab, int hidden, long long* token, const int* pos, void* x,
                      const void* rope_table, void* rope_cur, int rope_rows, int batch, void* stream);
int amq_decode_tail_suppress_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                                 const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids, void* stream);
int amq_decode_tail_batch_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                              const void* rope_table, void* rope_cur, int rope_rows, int batch, void* stream);

/* ---- sampled decoding ---------------------------------------------------------------------------------
 * Temperature / top-k / top-p sampling and EOS stop (what HF's `_sample` does with its logits warpers, torch.multinomial, unfinished_sequences
 * and pad filling -- amq/kernel/monkeypatch/ftllama_generate.py:257-325 -- between two token steps), as one launch that a captured step can end in.
 * Everything that may change between replays is read from ONE 128-byte device block, `state`, of 32 int32 words:
 *     word  0      float  temperature (> 0)
 *     word  1      int32  top_k (0 = off)
 *     word  2      float  top_p (>= 1 = off)
 *     word  3      int32  pad_id
 *     words 4-5    uint64 seed (low word first)
 *     words 6-7    uint64 draw counter (low word first); advanced by the kernel under AMQ_SAMPLE_ADVANCE
 *     words 8-15   int32  EOS token ids, -1 = unused slot
 *     words 16-23  int32  finished flag of sequence 0 .. 7 (0 = still generating)
 *     word  24     int32  number of unfinished sequences after the last launch with AMQ_SAMPLE_EOS (written by the kernel)
 *     word  25     int32  arrival ticket of the launch's workgroups: zero before the first launch, left zero by every launch
 *     word  26     int32  non-zero: no draw, u = 0 -- the first kept token in token order (with top_k = 1: the greedy arg-max, first maximum)
 *     words 27-31  reserved, zero
 * Per row, in HF's order: suppressed ids (suppress_ids: device int32 [8], -1 = unused, or NULL), NaN and -inf are no candidates;
 * z = logit / temperature; top-k keeps z >= the k-th largest value (ties with it all kept, TopKLogitsWarper); top-p keeps a token iff the
 * probability of the tokens with a STRICTLY larger logit is < top_p (TopPLogitsWarper with min_tokens_to_keep = 1, except that a tie class at the
 * boundary is kept whole where HF cuts inside it in sort order); u = (Philox4x32-10(key = seed, counter = {draw counter, sequence index, 0})[0] >> 8)
 * * 2^-24; the token is the first one, in ascending token index over the kept set, whose inclusive cumulative probability exceeds u * kept mass.
 * Weights are rounded once to 2^-40 fixed point and summed as integers: same inputs -> same token, in any launch order.  This is NOT
 * torch.multinomial's stream.
 * amq_sample_f16: logits fp16 [rows, vocab] contiguous (any row alignment) -> token_out int64 [rows]; row r is sequence seq0 + r.  u_in: float
 * [rows] in [0, 1) used instead of the generator, or NULL; kept_out: uint8 [rows, vocab] kept-set mask, or NULL.  flags: AMQ_SAMPLE_ADVANCE = the
 * draw counter is advanced by one after the launch; AMQ_SAMPLE_EOS (rows <= 8) = a finished sequence emits pad_id, one that draws an EOS id
 * emits it and becomes finished, word 24 is updated.  The state block must not be shared by launches that can run concurrently. */
#define AMQ_SAMPLE_ADVANCE 1
#define AMQ_SAMPLE_EOS 2
int amq_sample_f16(const void* logits, int rows, int vocab, void* state, const int* suppress_ids, const float* u_in, long long* token_out,
                   unsigned char* kept_out, int seq0, int flags, void* stream);
/* The end of a SAMPLED token step in one launch: the above for logits [batch, vocab] (batch <= 8, sequence index = row, both flags set), then
 * amq_decode_tail_suppress_f16's duties unchanged: token[b], pos += 1 (saturating at rope_rows), x[b] = embed[token[b]], rope_cur. */
int amq_decode_tail_sample_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                               const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids, void* state,
                               void* stream);

/* ---- evaluation metrics of the deployed model: row reductions over fp16 logits (amq_eval.hip) ----------------
 * One workgroup per row, fp32 arithmetic, a fixed summation order (per-thread serial sums, DPP wave reduce, waves in order through LDS; no
 * atomics): a row's result has the same bits launched alone or among others and does not depend on its index or alignment.  Rows may have any
 * alignment of their element type; strides are in ELEMENTS and >= V.  No synchronisation.  AMQ_EINVAL: null pointer, M < 1, V < 1, bad flag;
 * AMQ_ESHAPE: a stride shorter than a row.
 *
 * amq_logit_nll_f16: logits fp16 [M rows of V, row_stride apart]; labels int64 [M] on the device, or NULL (every row as if labelled -100).
 * Per row:   lse = max + log(sum_v exp(l[v] - max)),   nll = lse - float(l[label]),   argmax = index of the first maximum (int32).
 * label == -100 (HF's ignore_index): nll = 0, the caller counts the row out.  Any other label outside 0 .. V - 1: nll = NaN for that row; the
 * logit is not read.  nll_out float [M]; lse_out float [M] and argmax_out int32 [M] may be NULL. */
int amq_logit_nll_f16(const void* logits, long long row_stride, const long long* labels, int M, int V, float* nll_out, float* lse_out,
                      int* argmax_out, void* stream);
/* amq_logit_jsd_f16: p fp16 (this model's logits), q fp16 (q_is_f32 = 0) or fp32 (q_is_f32 = 1) (the dense model's), both [M rows of V].
 * Per row, the reference's JSD (amq/utils/loss.py: KLDivLoss with log_target against the clamped mixture) on fp32 values:
 *     lp = p - lse_p,   lq = q - lse_q,   m = log(max(0.5 * (e^lp + e^lq), eps)),
 *     jsd = 0.5 * sum_v [ e^lp * (lp - m) + e^lq * (lq - m) ]
 * Where the mixture is not clamped, lp - m and lq - m are evaluated from d = lq - lp as -log(0.5 (1 + e^d)) and d - log(0.5 (1 + e^d)): the same
 * values, without the half-ulp-at-log-V error that forming lp and m first would put into every term.
 * The clamp is part of the definition: identical rows score slightly NEGATIVE where entries fall below eps (about -2.4e-4 at V = 32000 with the
 * reference's eps = 1e-7).  Inputs are finite; what -inf logits give is unspecified.  jsd_out float [M]. */
int amq_logit_jsd_f16(const void* p, long long p_stride, const void* q, long long q_stride, int q_is_f32, int M, int V, float eps, float* jsd_out,
                      void* stream);

/* ---- sequences at positions of their OWN (batched decode over prompts of unequal length) ----------------
 * The batched entry points above keep ONE step state: every sequence is at the same position.  Here `step_states` is an ARRAY of `batch` blocks
 * with the layout of amq_attn_decode_cur_f16's block
 *     { fp16 cos/sin [64][2] of sequence b's CURRENT position ; int32 position at byte 256 ; int32 sticky error word at byte 260 ; pad }
 * AMQ_STEP_STATE_STRIDE bytes apart (block b at step_states + b * AMQ_STEP_STATE_STRIDE).  Sequence b occupies rows 0 .. pos[b] - 1 of its slice
 * of the caches -- a left-padded HF batch stored compactly: with position ids cumsum(mask) - 1 and the pad keys masked, HF's result for a row is
 * that of the row alone -- so no attention mask reaches a kernel.  Same kernels as the shared-position entry points, instantiated with the block
 * chosen by the sequence index: with equal positions in every block the results are theirs bit for bit. */
#define AMQ_STEP_STATE_STRIDE 272
/* RoPE + KV append + attention: sequence b rotates with block b's row, appends at row pos[b] and attends rows 0 .. pos[b].  n_splits == 0: one
 * workgroup per head (amq_attn_decode_cur_f16; workspace / tickets may be NULL); n_splits >= 1: amq_attn_decode_split_f16's kernels -- chunks follow
 * from each sequence's own position; grouped-query models take the matrix-core kernel and its combine launch as there; workspace (
 * amq_attn_decode_split_workspace_bytes) and tickets as there.  A sequence whose position is outside 0 .. max_seq-1 is a no-op for THAT sequence
 * and raises ITS block's error word; the others proceed. */
int amq_attn_decode_seq_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int batch,
                            int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                            void* tickets, void* stream);
/* amq_decode_tail_suppress_f16 (suppress_ids may be NULL: none) with every sequence advancing ITS position (saturating at rope_rows) and writing ITS
 * cos/sin row: token[b] = argmax(logits[b]), pos[b] += 1, x[b] = embed[token[b]], row[b] = rope_table[min(pos[b], rope_rows - 1)]. */
int amq_decode_tail_seq_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                            const void* rope_table, int rope_rows, int batch, const int* suppress_ids, void* stream);
/* amq_decode_tail_sample_f16 likewise (draw (seed, i, b) and EOS bookkeeping unchanged; batch <= 8). */
int amq_decode_tail_sample_seq_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                                   const void* rope_table, int rope_rows, int batch, const int* suppress_ids, void* state, void* stream);
/* amq_set_token_f16 likewise: row[b] = rope_table[min(pos[b], rope_rows - 1)]; the positions are not changed. */
int amq_set_token_seq_f16(const long long* token_in, int n_in, const void* embed, int vocab, int hidden, long long* token, void* step_states, void* x,
                          const void* rope_table, int rope_rows, int batch, void* stream);

/* ---- prompt-lookup speculative decoding (greedy, one sequence): a step over R = D + 1 consecutive positions ------------------------------
 * Row 0 of a step is the sequence's current token at position p, rows 1 .. D are guessed continuations (drafts) at p + 1 .. p + D.  One pass of
 * the weights over the R rows (the 2 .. 8-row GEMV routes) verifies them all; the step emits 1 + (accepted drafts) tokens and is by construction
 * a greedy decode.  step_states: R blocks of the amq_*_seq_f16 layout, block j holding position p + j and its cos/sin row.
 *
 * amq_attn_decode_rows_f16: amq_attn_decode_seq_f16 for `rows` (2 .. 8) rows of ONE sequence -- q / k / v / out have `rows` rows, there is ONE cache
 * slice [n_kv_heads, max_seq, 128].  Row j rotates with block j, appends its K / V at cache row p + j and attends cache rows 0 .. p - 1 plus this
 * step's rows 0 .. j (causal among the rows): every workgroup rotates the earlier rows of the step itself from k / v (they are being appended by
 * other workgroups of the same launch and are never read from the cache).  Read from a cache that already holds rows p .. p + j - 1, row j's output
 * is amq_attn_decode_seq_f16's at position p + j bit for bit (n_splits == 0: one workgroup per (head, row); n_splits >= 1: the per-head split kernel,
 * chunks from each row's own position, bit-identical with one active chunk; grouped-query models take the per-head kernels here too --
 * their matrix-core form is amq_attn_decode_rows_gqa_f16 below).  workspace
 * (amq_attn_decode_split_workspace_bytes(rows, ...)) and tickets [rows * n_heads] as there.  A row whose position is outside 0 .. max_seq-1 (or whose
 * row 0 would be below 0) is a no-op for THAT row and raises ITS block's error word.  Rows of rejected drafts stay in the cache behind the new
 * position; no step reads them before a later step overwrites them. */
#define AMQ_LOOKUP_MAX_ROWS 8
int amq_attn_decode_rows_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int rows,
                             int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                             void* tickets, void* stream);
/* amq_attn_decode_rows_f16 for GROUPED-QUERY models (2 <= n_heads / n_kv_heads <= 16, else AMQ_ESHAPE) on the matrix cores: the same arguments, rows,
 * appends, causal rule among the rows and out-of-range behaviour (p < 0: every row is a no-op and raises its block's error word).  One workgroup per
 * (kv head, block of 16 query rows, chunk) takes the chunk's K / V in once and scores it against its query rows -- query row (j, g) = step row j,
 * head g of the group -- with amq_attn_decode_seq_f16's grouped kernel's slicing and orders, the key limit per query row: row j's output and the
 * cache rows p .. p + rows - 1 are, bit for bit, what `rows` successive amq_attn_decode_seq_f16 calls (batch 1, the same n_splits >= 2) at positions
 * p .. p + rows - 1 leave.  n_splits: 1 .. 1024 chunks of 128 * ceil(ceil(max_seq / n_splits) / 128) keys (0: AMQ_EINVAL); workspace (
 * amq_attn_decode_split_workspace_bytes(rows, n_heads, n_splits)) is required; tickets must be given and is not used (the rows are finished by the
 * grouped kernel's combine launch). */
int amq_attn_decode_rows_gqa_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int rows,
                                 int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                                 void* tickets, void* stream);
/* The verify-and-propose tail, one launch.  lookup_state: a device block of AMQ_LOOKUP_STATE_WORDS int32 words, all of them read (and the counters
 * written) on every launch, so a captured step never needs a re-capture:
 *   word 0      D: drafts per step (1 .. 7; the launch's rows = D + 1)
 *   word 1      ngram_max: longest suffix looked up (1 .. 4)
 *   word 2      mode: 0 = the tail proposes the next drafts from the history; 1 = external drafts (the tail writes -1 drafts; the host fills rows
 *               1 .. D with amq_set_token_seq_f16 over `rows` blocks and writes the unclamped ids into words 9 .. 8 + D)
 *   word 3      tokens in `history` (prompt + everything emitted; the sequence's current token is the last one)
 *   word 4      steps taken (incremented by every launch)
 *   word 5      n: drafts accepted by the last step
 *   word 6      ticket of the last-arriver protocol: zero before and after every launch
 *   word 7      reserved (0)
 *   words 8+j   j = 1 .. 7: the draft row j of the NEXT step runs with, unclamped (-1 = no draft: never accepted); word 8 unused
 *   words 16+j  j = 0 .. 7: arg-max of row j of the last step
 *   words 24..  reserved (0)
 * a[j] = argmax(logits[j]) (first maximum; suppress_ids -- int32 [8], -1 = unused, or NULL -- left out in every row).  n = the largest value with
 * draft[i] == a[i - 1] for all 1 <= i <= n; a[0 .. n] are appended to history (int32 [history_cap], history_cap >= rope_rows) and the counters advance.
 * Proposal: for g = ngram_max .. 1, the MOST RECENT earlier occurrence in history of its last g tokens that is followed by at least one token; the
 * drafts are the up to D tokens behind it, unfilled slots -1.  Then token[0] = a[n], token[j] = draft j clamped into the vocabulary, x[j] =
 * embed[token[j]], block j's position = (block 0's position + n + 1) + j saturating at rope_rows, and its cos/sin row. */
#define AMQ_LOOKUP_STATE_WORDS 32
int amq_decode_tail_lookup_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                               const void* rope_table, int rope_rows, int rows, const int* suppress_ids, void* lookup_state, int* history,
                               int history_cap, void* stream);
/* The SAMPLED verify-and-propose tail, one launch: amq_decode_tail_lookup_f16 with a[j] DRAWN from row j instead of its arg-max.  Row j runs
 * amq_sample_f16's sampler (the same kept set, weights and ascending-index draw; suppress_ids are never drawn; a row without a candidate gives
 * token 0) with the parameters of sample_state, the 128-byte block of amq_sample_f16:
 *   read      words 0 .. 2 (temperature, top_k, top_p), words 4 .. 5 (seed), words 6 .. 7 (the 64-bit draw counter c), word 26 (first_kept)
 *   advanced  words 6 .. 7: c + n + 1 (64-bit), by the last workgroup to arrive -- every workgroup has read c before it takes its ticket
 *   untouched the pad id, the EOS ids, the finished flags, the unfinished count and the arrival word (25: stays 0): there is NO EOS bookkeeping
 *             here -- the host finds the first EOS id in `history`
 * Row j's uniform number is Philox(seed; draw = c + j (64-bit add), sequence 0): the token emitted at index i of the sequence (0 = the first one
 * after the prompt) is drawn with counter i whichever row of whichever step computes it -- the numbers amq_decode_tail_sample_f16 uses for a
 * single sequence.  Acceptance, history, counters, proposal and the next step's inputs are amq_decode_tail_lookup_f16's with the drawn tokens in
 * the place of the arg-maxes; words 16 + j of lookup_state hold the DRAWN token of row j.
 * u_in (float32 [rows] or NULL): uniform numbers used instead of the generator; kept_out (uint8 [rows, vocab] or NULL): the kept-set masks.
 * The checks of amq_decode_tail_lookup_f16; sample_state NULL: AMQ_EINVAL. */
int amq_decode_tail_lookup_sample_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                                      const void* rope_table, int rope_rows, int rows, const int* suppress_ids, void* lookup_state, int* history,
                                      int history_cap, void* sample_state, const float* u_in, unsigned char* kept_out, void* stream);

/* ---- many-row (prefill) glue --------------------------------------------------------------------------
 * The reference runs these steps as framework ops between the linears of a HF Llama block
 * (transformers LlamaAttention / LlamaMLP / LlamaDecoderLayer as driven by amq/utils/speed.py:150-200); on this path
 * they are ~20 tiny launches per block, so they are offered fused. */

/* amq_gemm_splitk_f16 plus a fused residual: y = residual + fp16(x . W^T (+ bias)); residual fp16 [M, y_stride] or
 * NULL, may alias y.  workspace NULL = single pass (no split-K).  x_stride / y_stride: the row-stride rule at amq_gemv_f16 (0, or >= K / N and % 8 == 0). */
int amq_gemm_res_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                     const void* bias, const void* residual, void* y, int M, int N, int K, int group, int x_stride,
                     int y_stride, void* workspace, size_t workspace_bytes, void* stream);
/* amq_gemm_res_f16 (dense y) followed by amq_rmsnorm_xfrag_f16 of its result rows -- y = residual + fp16(x . W^T (+ bias)), xf = the fragment-ordered
 * gamma * fp16(y * rsqrt(mean(y^2) + eps)) -- as ONE call: where the GEMM runs split-K (few rows, a workspace given) the sum over the splits and the
 * norm are one launch, otherwise the norm follows as its own.  Same bits as the two calls.  N % 128 == 0; xf: amq_xfrag_bytes(M, N) bytes.
 * The hand-over between a decoder block's down_proj and the next block's input_layernorm on a short prompt pass (the reference runs both as
 * separate framework ops: transformers LlamaDecoderLayer as driven by amq/utils/speed.py:150-200).  (ABI 521) */
int amq_gemm_res_norm_xfrag_f16(int bits, int mode, const void* x, const void* qweight_native, const void* meta_native, const void* bias,
                                const void* residual, void* y, int M, int N, int K, int group, int x_stride, void* workspace,
                                size_t workspace_bytes, const void* gamma, float eps, void* xf, void* stream);
/* The same with the kernel family chosen by the caller (tests, A/B tools); amq_gemm_route_workspace_bytes is the
 * matching workspace query (0: no workspace needed).  The workspace holds split-K partials (few rows) or the dequantized
 * fp16 weights (AMQ_GEMM_DEQ, and AUTO on MFMA-bound launches) -- never both; without it AUTO runs a fused kernel.
 * x_stride / y_stride: the same row-stride rule for every route (0, or >= K / N and % 8 == 0). */
size_t amq_gemm_route_workspace_bytes(int route, int M, int N, int K);
/* ... for a given group size: groups of 64 / 32 take the few-row kernel up to 256 rows (0 bytes), the tiled kernel beyond (split-K partials as for
 * group 128) and the dequantize-once route (N * K * 2 bytes) for launches that fill 256 x 256 tiles -- the ring / wave-specialised kernels read one
 * (scale, zero) pair per 128 columns. */
size_t amq_gemm_route_workspace_bytes_g(int route, int M, int N, int K, int group);
int amq_gemm_route_f16(int route, int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                       const void* bias, const void* residual, void* y, int M, int N, int K, int group, int x_stride,
                       int y_stride, void* workspace, size_t workspace_bytes, void* stream);
/* y = x . W^T (+ bias) (+ residual | silu-gated) with W as DENSE fp16 [N, K] (row-major): the matmul of GPTQLinear.forward's
 * many-row branch (hqq/backends/autogptq.py:283: torch.matmul(x, weights)) as a hand-written kernel -- what AMQ_GEMM_DEQ runs
 * behind amq_dequantize_f16, exported for callers that keep fp16 weights (lm_head, an fp16 base model).  N % 16 == 0,
 * K % 128 == 0, x_stride % 8 == 0, y_stride % 4 == 0 (0 = dense; else x_stride >= K, y_stride >= N); epilogue operands as amq_gemm_res_f16 /
 * amq_gemm_gated_f16. */
int amq_gemm_f16w_f16(const void* x, const void* w_f16, const void* bias, const void* residual, const void* gate, void* y,
                      int M, int N, int K, int x_stride, int y_stride, void* stream);
/* The LlamaMLP product act_fn(gate_proj(x)) * up_proj(x) with up_proj as this GEMM:
 *     y = fp16(silu(gate)) * fp16(x . W^T (+ bias)),   gate fp16 [M, N] contiguous, y [M, N] contiguous,
 * formed in the epilogue of the kernel that serves the shape (256-row ring and few-row kernels) or by the element-wise
 * launch behind it (tiled kernel) -- the same expression as amq_silu_mul_f16 on the separate outputs, bit for bit.
 * gate may alias y only in the first case: amq_gemm_gated_fused(route, M, N, K, use_workspace) says which it is
 * (use_workspace: whether a split-K workspace will be passed).  route / workspace as amq_gemm_route_f16; x_stride: 0, or >= K and % 8 == 0. */
int amq_gemm_gated_fused(int route, int M, int N, int K, int use_workspace);
int amq_gemm_gated_fused_g(int route, int M, int N, int K, int use_workspace, int group);   /* ... for a given group size (64 / 32: few-row kernel and dequantize-once yes, tiled no) */
int amq_gemm_gated_f16(int route, int bits, int mode, const void* x, const void* qweight_native, const void* meta_native,
                       const void* bias, const void* gate, void* y, int M, int N, int K, int group, int x_stride,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Fragment-ordered activations for few-row GEMMs.  For a few dozen rows the GEMM is bound by how fast a CU can pull x
 * in MFMA operand order; amq_xfrag_f16 lays x out so that every wave-load is one contiguous KiB that already IS an
 * operand:  xf[g][kt][mb*4 + t][lane = 16*o + r][8] = x[g*64 + mb*16 + r][kt*128 + 32*t + 8*o .. +8]  (rows >= M zero),
 * amq_xfrag_bytes(M, K) bytes.  Source element (m, k) is read at src[m*stride_m + (k/128)*stride_kt + k%128] (halves):
 * row-major [M, K]: stride_m = K (or more), stride_kt = 128; an attention output [heads, M, 128]: 128, M*128.
 * amq_gemm_xfrag_f16 = amq_gemm_res_f16 reading such a buffer (any M; no workspace), plus an optional SiLU gate. */
size_t amq_xfrag_bytes(int M, int K);
int amq_xfrag_f16(const void* src, void* xf, int M, int K, long long stride_m, long long stride_kt, void* stream);
/* amq_rmsnorm_f16 (rows of K, contiguous) writing its result in fragment order */
int amq_rmsnorm_xfrag_f16(const void* x, const void* gamma, void* xf, int M, int K, float eps, void* stream);
/* gate (fp16 [M, y_stride] or NULL, may alias y): y = fp16(silu(gate)) * fp16(x . W^T (+ bias)) -- the LlamaMLP product
 * act_fn(gate_proj(x)) * up_proj(x) formed in up_proj's epilogue (same expression as amq_silu_mul_f16).  y_stride (also the gate's and the
 * residual's): 0, or >= N and % 8 == 0 */
int amq_gemm_xfrag_f16(int bits, int mode, const void* xf, const void* qweight_native, const void* meta_native,
                       const void* bias, const void* gate, const void* residual, void* y, int M, int N, int K, int group,
                       int y_stride, void* stream);
/* Several linears over the SAME fragment-ordered x (q/k/v, gate/up of a prompt pass), each with its own bit-width, as
 * segments of one few-row launch (amq_segment as for amq_gemv_grouped_f16; residual optional per segment):
 * y_i = x . W_i^T (+ bias_i) (+ residual_i).  Results are those of amq_gemm_xfrag_f16 per segment, bit for bit.  Every segment's y_stride: 0, or
 * >= its N and % 8 == 0. */
int amq_gemm_xfrag_grouped_f16(const amq_segment* segments /* host */, int nseg, const void* xf, int M, int K, int group,
                               void* stream);
/* The same launch with its kernel form chosen by the caller (tests, A/B tools; the results do not depend on it, bit for bit):
 * AMQ_FEWROW_AUTO = what amq_gemm_xfrag_grouped_f16 runs (the streaming form where it saves a round of the chip), AMQ_FEWROW_TILE = x fragments a
 * whole K tile at a time (up to four 16-column blocks per workgroup), AMQ_FEWROW_STREAM = one MFMA step at a time through a register ring
 * (amq_gemm_fewrow.hip; blocks_per_wg 1, 2, 3, 4 or 6; 0 = by the launch's size). */
#define AMQ_FEWROW_AUTO   0
#define AMQ_FEWROW_TILE   1
#define AMQ_FEWROW_STREAM 2
int amq_gemm_xfrag_grouped_form_f16(const amq_segment* segments /* host */, int nseg, const void* xf, int M, int K, int group,
                                    int form, int blocks_per_wg, void* stream);
/* Causal self-attention over a prompt: for every sequence b < batch, query row s < S (position pos0 + s) and head h,
 *     out[b, s, h, :] = softmax(q[b, s, h, :] . K[b, 0 .. pos0 + s, g, :]^T / sqrt(128)) . V[b, 0 .. pos0 + s, g, :],   g = h / (n_heads / n_kv_heads)
 * as one flash-style MFMA kernel (fp32 scores and softmax, fp16 probabilities, like the eager HF path).  q must already be
 * rotated (amq_rope_cache_f16 / amq_rope_rows_f16), k rotated keys.  Layouts are given by strides in halves (multiples of 8):
 * element (b, s, h, d) of q / out at b*bstride + s*rstride + h*128 + d; key / value row t of kv head g at
 * b*bstride + t*rstride + g*hstride + d -- so the KV cache [n_kv_heads, max_seq, 128] (rstride 128, hstride max_seq*128) and
 * a projection output [rows, n_kv_heads*128] (rstride n_kv_heads*128, hstride 128) are both read in place, and out can be the
 * [rows, n_heads*128] matrix o_proj consumes.  Replaces the eager attention of the reference's prefill branch
 * (amq/kernel/monkeypatch/ftllama_modeling.py:88-126). */
int amq_attn_prefill_f16(const void* q, const void* k, const void* v, void* out, int batch, int S, int pos0, int n_heads,
                         int n_kv_heads, int head_dim, long long q_rstride, long long q_bstride, long long k_rstride,
                         long long k_bstride, long long k_hstride, long long v_rstride, long long v_bstride, long long v_hstride,
                         long long o_rstride, long long o_bstride, void* stream);
/* The same for ONE sequence with the result written in fragment order (amq_xfrag_f16's layout of the [S, n_heads * 128]
 * matrix; rows S .. 64 ceil(S / 64) - 1 zero): what o_proj's few-row GEMM (amq_gemm_xfrag_f16) reads, without the
 * re-ordering launch in between.  out_xf: amq_xfrag_bytes(S, n_heads * 128) bytes. */
int amq_attn_prefill_xfrag_f16(const void* q, const void* k, const void* v, void* out_xf, int S, int pos0, int n_heads,
                               int n_kv_heads, int head_dim, long long q_rstride, long long k_rstride, long long k_hstride,
                               long long v_rstride, long long v_hstride, void* stream);
/* The two decode-step restructurings that were built, proven bit-identical and measured SLOWER than the five-launch step -- q / k / v +
 * attention as one launch (amq_gemv_qkv_attn_f16) and one persistent launch per token (amq_decode_engine_*) -- are A/B routes: they are
 * declared in include/amq_hip_ab.h and exported by libamq_hip_ab.so (`make -C amq_amd/csrc ab`), not by this library. */

/* RoPE + KV-cache write for S new rows at positions pos0 .. pos0+S-1 of ONE sequence: q fp16 [S, n_heads*128] is
 * rotated in place; k [S, n_kv_heads*128] is rotated into kcache[h][pos0+s][:], v copied into vcache (both
 * [n_kv_heads, max_seq, 128]); rope_table from amq_rope_table_f16 (rows past rope_rows-1 clamp).  Same numerics as the
 * rotation inside amq_attn_decode_f16. */
int amq_rope_cache_f16(void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                       int rope_rows, int pos0, int S, int n_heads, int n_kv_heads, int head_dim, int max_seq, void* stream);
/* The same for `batch` sequences of S rows each in one launch: q [batch*S, n_heads*128], k / v [batch*S, n_kv_heads*128],
 * caches [batch, n_kv_heads, max_seq, 128]; row s belongs to sequence s / S at position pos0 + s % S.  (The prompt pass of a
 * batched decode runner; counterpart of the per-sequence loop the reference's batch-1 FT cache forces,
 * amq/kernel/monkeypatch/ftllama_modeling.py:61-68.) */
int amq_rope_cache_batch_f16(void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                             int rope_rows, int pos0, int S, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                             void* stream);
/* RoPE in place on q [rows, n_heads*128] and k [rows, n_kv_heads*128] for rows = batch * seq_len (no cache write):
 * position of row s = pos0 + s % seq_len.  For the batched prompt pass of the harness' GeMM mode (amq/utils/speed.py:61-71
 * with batch_size > 1, BASELINE.json configs[3]). */
int amq_rope_rows_f16(void* q, void* k, const void* rope_table, int rope_rows, int pos0, int rows, int seq_len, int n_heads,
                      int n_kv_heads, int head_dim, void* stream);
/* ---- per-head q / k RMSNorm in front of the rotation (Qwen3) ------------------------------------------------------------------------
 * Qwen3 applies an RMSNorm over the 128 values of every head of q and of k before the rotation (q_norm / k_norm: one fp16 [128] weight each,
 * shared by all heads of a layer).  The amq_*_qkn_f16 entry points are the rotating entry points above with that norm inside the same kernel:
 * x' = gamma * fp16(x * rsqrt(mean(x^2) + eps)) (fp32 statistic, one fp16 rounding, fp16 multiply: HF's Qwen3RMSNorm, amq_rmsnorm_f16's
 * arithmetic), then the unchanged fp16 rotation.  The statistic is one fixed summation tree in every kernel, so the key row a prompt pass writes,
 * the row a decode step appends (per-head, split, grouped-query kernel) and the row a `rows` workgroup rotates for itself have the same bits.
 * `norm`: host struct, device pointers; q_gamma and k_gamma both set.  norm == NULL: the entry point without the suffix, unchanged.
 * Every other argument, result and error as documented for the entry point of the same name. */
typedef struct amq_qk_norm {
    const void* q_gamma;      /* fp16 [128] */
    const void* k_gamma;      /* fp16 [128] */
    float eps;
} amq_qk_norm;
int amq_attn_decode_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                            const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                            int max_seq, float rope_theta, const void* rope_table, void* stream);
int amq_attn_decode_cur_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                const void* step_state, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                void* stream);
int amq_attn_decode_split_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                  const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads,
                                  int head_dim, int max_seq, float rope_theta, const void* rope_table, int n_splits,
                                  void* workspace, size_t workspace_bytes, void* tickets, void* stream);
int amq_attn_decode_seq_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                void* step_states, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                void* workspace, size_t workspace_bytes, void* tickets, void* stream);
int amq_attn_decode_rows_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                 void* step_states, int rows, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                 void* workspace, size_t workspace_bytes, void* tickets, void* stream);
int amq_attn_decode_rows_gqa_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                     void* step_states, int rows, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                     void* workspace, size_t workspace_bytes, void* tickets, void* stream);
/* amq_rope_cache_batch_f16 (batch 1: amq_rope_cache_f16) and amq_rope_rows_f16 with the heads of q and k normalised first */
int amq_rope_cache_qkn_f16(const amq_qk_norm* norm, void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                           int rope_rows, int pos0, int S, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                           void* stream);
int amq_rope_rows_qkn_f16(const amq_qk_norm* norm, void* q, void* k, const void* rope_table, int rope_rows, int pos0, int rows, int seq_len,
                          int n_heads, int n_kv_heads, int head_dim, void* stream);

/* out = fp16(silu(gate)) * up elementwise, n fp16 elements (n % 8 == 0): the LlamaMLP activation between up/gate and down */
int amq_silu_mul_f16(const void* gate, const void* up, void* out, size_t n, void* stream);

/* ---- bfloat16 variants (optional) ------------------------------------------------------------------
 * For models quantized with compute_dtype = torch.bfloat16: HQQLinear keeps scale / zero in the compute dtype and dequantizes in it
 * (hqq/core/quantize.py:184-199, 396-407, 516), W = bf16(bf16(q - zero) * scale).  The native payload is the fp16 path's; the meta words hold
 * bfloat16 (scale, zero) pairs -- amq_repack_from_hqq copies 16-bit patterns, so it repacks a bf16 model as it stands.  A native buffer repacked from
 * bf16 meta must only be given to the *_bf16 entry points (and one repacked from fp16 meta only to the *_f16 ones): the meta carries no dtype tag.
 * AMQ_MODE_HQQ arithmetic and groups of 128 (or multiples) only: the reference's GPTQ / AWQ kernels are fp16-only (hqq/backends/ft.py:62).
 * x, bias, residual, y, W_out: bfloat16.  Weights bit-identical to Quantizer.dequantize; fp32 accumulation, one bf16 rounding of y, bias and residual as
 * separate bf16 adds. */
int amq_dequantize_bf16(int bits, const void* qweight_native, const void* meta_native_bf16, int N, int K, int group, void* W_out, void* stream);
/* Format A with bfloat16 scale / zero -> W[N,K] bfloat16: Quantizer.dequantize under compute_dtype = bfloat16 as one kernel (any group amq_dequantize_hqq_f16 takes) */
int amq_dequantize_hqq_bf16(int bits, const void* W_q, const void* scale, const void* zero, int N, int K, int group, void* W_out, void* stream);
/* 1 .. 16 rows: weight-streaming kernel (unpacked block = MFMA operand, v_mfma_f32_16x16x32_bf16); x_stride / y_stride in elements (0 = dense;
 * x_stride a multiple of 8: rows are read in 16-byte pieces).  residual (or null): y = residual + (x W^T + bias), bfloat16 [M, y_stride], may alias y */
int amq_gemv_bf16(int bits, const void* x, const void* qweight_native, const void* meta_native_bf16, const void* bias, const void* residual, void* y,
                  int M, int N, int K, int group, int x_stride, int y_stride, void* stream);
/* any M: up to 16 rows amq_gemv_bf16; beyond, dequantize once into `workspace` (>= amq_gemm_bf16_workspace_bytes(M, N, K) bytes = N * K * 2 from 17 rows)
 * and multiply with the bf16 instantiation of the MFMA-bound GEMM kernel (amq_gemm_f16.hip); x_stride % 8 == 0 and y_stride % 4 == 0 there */
size_t amq_gemm_bf16_workspace_bytes(int M, int N, int K);
int amq_gemm_bf16(int bits, const void* x, const void* qweight_native, const void* meta_native_bf16, const void* bias, const void* residual, void* y,
                  int M, int N, int K, int group, int x_stride, int y_stride, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMQ_HIP_H */
