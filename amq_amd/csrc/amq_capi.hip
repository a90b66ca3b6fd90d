// amq_capi.hip -- extern "C" boundary of libamq_hip.so (see include/amq_hip.h).
// Argument validation + dispatch only; no allocation, no synchronisation.
#include "../../include/amq_hip.h"
#ifdef AMQ_AB_ROUTES
#include "../../include/amq_hip_ab.h"
#endif
#include "amq_common.cuh"
#include "amq_kernels.h"

#include <stdarg.h>
#include <stdio.h>
#include <vector>

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return AMQ_OK;
    return fail(AMQ_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// 128, or a multiple of it that divides K: the repack entry points read such a source format and replicate each group's
// (scale, zero) into the native layout's per-128 pairs; the compute entry points work on the native layout either way
// 64 / 32: the native meta holds 128 / group pairs per (row, tile) (amq_common.cuh); served by the repack / dequantize entry points, the GEMV
// kernel (<= 16 rows, exact math) and the dequantize-once GEMM route -- the other entry points refuse them (check_shape128)
int check_group(int group) {
    if (group != 64 && group != 32 && (group < 128 || (group % 128) != 0))
        return fail(AMQ_ESHAPE, "group size must be 32, 64 or a multiple of 128 (got %d)", group);
    return AMQ_OK;
}
int check_shape(int bits, int N, int K, int group) {
    if (bits != 2 && bits != 3 && bits != 4) return fail(AMQ_EINVAL, "bits must be 2, 3 or 4 (got %d)", bits);
    if (int rc = check_group(group)) return rc;
    if (N <= 0 || K <= 0 || (N % 16) != 0 || (K % 128) != 0)
        return fail(AMQ_ESHAPE, "need N %% 16 == 0 and K %% 128 == 0 (got N=%d K=%d)", N, K);
    if ((K % group) != 0) return fail(AMQ_ESHAPE, "group size %d does not divide K=%d", group, K);
    return AMQ_OK;
}

// entry points whose kernels read ONE (scale, zero) pair per (row, 128-column tile)
int check_shape128(int bits, int N, int K, int group, const char* who) {
    if (group == 64 || group == 32)
        return fail(AMQ_ESHAPE, "%s serves groups of 128 (and multiples); groups of %d run through amq_gemv_f16 / amq_gemv_grouped_f16 (<= 16 rows) and "
                    "amq_gemm_route_f16 / amq_gemm_gated_f16 with a workspace of N * K * 2 bytes", who, group);
    return check_shape(bits, N, K, group);
}

int check_mode(int mode) {
    if (mode != AMQ_MODE_HQQ && mode != AMQ_MODE_FMA && mode != AMQ_MODE_FMA1) return fail(AMQ_EINVAL, "unknown dequant mode %d", mode);
    return AMQ_OK;
}
// AMQ_MODE_FMA1 (scales within amq_fma1_scale_bound: the GEMV kernel's one-op unpack) is AMQ_MODE_FMA to every other kernel: the same results
int kernel_mode(int mode) { return mode == AMQ_MODE_FMA1 ? AMQ_MODE_FMA : mode; }

constexpr size_t LDS_LIMIT = 160 * 1024;

// Row strides of the fp16 matmul entry points, in elements as the caller passed them (0 = dense; an entry point without one of the two passes 0).
// What the kernels behind them assume, none of which they can check themselves:
//   - a stride is at least the row it steps over (a shorter or negative one makes rows overlap, or walks backwards out of the buffer);
//   - x rows are read in 16-byte pieces (amq_gemm.hip issue_a / skinny_body, amq_gemv_body.cuh stage_x / x_dma_rows -- x2 of the SiLU*mul / mul
//     prologues at x's stride --, amq_gemm_ring.hip, amq_gemm_ws.hip, amq_gemm_f16.hip): x_stride % 8;
//   - y and the residual are accessed in pieces of up to 16 bytes at row * y_stride + 8 j (the split-K reduce kernels of amq_gemm.hip; 8 bytes in the
//     ring / wave-specialised / fp16-weight epilogues): y_stride % y_align, 8 for every entry point that can reach the reduce, 4 for amq_gemm_f16w_f16;
//   - the few-row GEMM kernel (up to x_i32_rows rows; 0: not reachable) forms its x offsets row * x_stride + column as 32-bit ints.
// Dense calls cannot fail the alignment rules: K % 128 == 0 and N % 16 == 0 are required of every call.
int check_strides(const char* who, int M, int K, int x_stride, int N, int y_stride, int y_align, int x_i32_rows) {
    if (x_stride < 0 || (x_stride != 0 && x_stride < K))
        return fail(AMQ_ESHAPE, "%s: x_stride=%d is shorter than a row of x (K=%d); 0 = dense", who, x_stride, K);
    if (y_stride < 0 || (y_stride != 0 && y_stride < N))
        return fail(AMQ_ESHAPE, "%s: y_stride=%d is shorter than a row of y (N=%d); 0 = dense", who, y_stride, N);
    if (x_stride & 7) return fail(AMQ_ESHAPE, "%s: x_stride=%d must be a multiple of 8 elements (rows of x are read in 16-byte pieces)", who, x_stride);
    if (y_stride % y_align)
        return fail(AMQ_ESHAPE, "%s: y_stride=%d must be a multiple of %d elements (rows of y and of the residual are accessed in %d-byte pieces)", who,
                    y_stride, y_align, 2 * y_align);
    if (x_stride > K && M >= 1 && M <= x_i32_rows && (long long)(M - 1) * x_stride + K > 0x7fffffffll)
        return fail(AMQ_ESHAPE, "%s: x_stride=%d: %d strided rows of x span 2^31 elements or more (the few-row kernel's offsets are 32-bit)", who, x_stride, M);
    return AMQ_OK;
}
// "<entry point>, segment i" for the messages of the grouped calls
const char* seg_name(const char* who, int i) {
    static thread_local char buf[96];
    snprintf(buf, sizeof(buf), "%s, segment %d", who, i);
    return buf;
}
constexpr int FEWROW_MAX_ROWS = 256;       // rows the few-row GEMM kernel can be given (64; 256 with groups of 64 / 32: gemm_fine_takes_skinny)
// ... on a route call: a forced tiled / ring / wave-specialised route never ends in the few-row kernel (amq_gemm.hip gemm_is_skinny; a ring call that
// gemm_ring_ok turns away runs the tiled kernel, whose x offsets are size_t), and AMQ_GEMM_DEQ runs the fp16-weight GEMM or is refused (gemm_f16w_ok
// holds x below 4 GiB itself); AUTO and SKINNY can
int fewrow_rows_of(int route) {
    return (route == AMQ_GEMM_AUTO || route == AMQ_GEMM_SKINNY) ? FEWROW_MAX_ROWS : 0;
}

}  // namespace

extern "C" {

int amq_version(void) { return AMQ_VERSION; }
const char* amq_last_error(void) { return g_err; }

int amq_query(int K, int* out, int cap) {
    int vals[6];
    int maxm = 0, maxm_plain = 0, maxm_plain_nonorm = 0;
    for (int m = 1; m <= amq::GEMV_MAX_M; ++m) {
        if (amq::gemv_min_lds_bytes(m, K, false) <= LDS_LIMIT) maxm = m;
        if (amq::gemv_min_lds_bytes(m, K, true, true) <= LDS_LIMIT) maxm_plain = m;
        if (amq::gemv_min_lds_bytes(m, K, true, false) <= LDS_LIMIT) maxm_plain_nonorm = m;
    }
    vals[0] = maxm;                 // largest M amq_gemv_f16 / amq_gemv_grouped_f16 accept for this K whatever the options and group size
    vals[1] = (int)LDS_LIMIT;
    vals[2] = amq::TILE_N;
    vals[3] = amq::TILE_K;
    vals[4] = maxm_plain;           // ... with default options over groups of 128 (2 .. 8 rows run kernels with a smaller cross-wave sum buffer)
    vals[5] = maxm_plain_nonorm;    // ... and no RMSNorm prologue (x may then be staged in two K phases: 8 rows at K = 11008)
    int n = cap < 6 ? cap : 6;
    for (int i = 0; i < n; ++i) out[i] = vals[i];
    return n;
}

size_t amq_native_qweight_bytes(int bits, int N, int K) { return amq::native_qweight_bytes(bits, N, K); }
float amq_fma1_scale_bound(int bits) { return (bits == 2 || bits == 3 || bits == 4) ? amq::fma1_scale_bound(bits) : 0.0f; }
size_t amq_native_meta_bytes(int N, int K, int group) { return amq::native_meta_bytes(N, K, group > 0 ? amq::meta_pairs(group) : 1); }

int amq_repack_from_hqq(int bits, const void* W_q, const void* scale, const void* zero, int N, int K, int group,
                        void* qn, void* mn, void* stream) {
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (!W_q || !scale || !zero || !qn || !mn) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_repack(amq::FMT_HQQ, bits, W_q, scale, zero, N, K, qn, mn, (hipStream_t)stream, group), "repack_from_hqq");
}

int amq_repack_from_gptq(int bits, const void* qweight, const void* scales, const void* zeros, int N, int K, int group,
                         void* qn, void* mn, void* stream) {
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (!qweight || !scales || !zeros || !qn || !mn) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_repack(amq::FMT_GPTQ, bits, qweight, scales, zeros, N, K, qn, mn, (hipStream_t)stream, group), "repack_from_gptq");
}

int amq_repack_from_awq(const void* qweight, const void* scales, const void* scaled_zeros, int N, int K, int group,
                        void* qn, void* mn, void* stream) {
    if (int rc = check_shape(4, N, K, group)) return rc;
    if (!qweight || !scales || !scaled_zeros || !qn || !mn) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_repack(amq::FMT_AWQ, 4, qweight, scales, scaled_zeros, N, K, qn, mn, (hipStream_t)stream, group), "repack_from_awq");
}

// The quantizer family's one validator.  A family is what its kernels are instantiated for and how it words a refused group: HQQ's solve takes
// four group sizes and wants the group to divide K; the GPTQ solve and AWQ's kernels take the three that fit a 128-column block (a multiple of
// 128 they all divide), and the GPTQ solve says why 256 is not among them.  T: the rows of activations (1 for the calls without any).
struct QuantFamily { const char* serves; bool has256, explains256; };
constexpr QuantFamily QUANT_HQQ = {"the quantizer serves groups of 32, 64, 128 and 256", true, false};
constexpr QuantFamily QUANT_GPTQ = {"the GPTQ solve serves groups of 32, 64 and 128", false, true};
constexpr QuantFamily QUANT_AWQ = {"the AWQ kernels serve groups of 32, 64 and 128", false, false};

static int check_quantize_shape(const QuantFamily& f, int bits, int N, int K, int group, int T = 1) {
    if (bits != 2 && bits != 3 && bits != 4) return fail(AMQ_EINVAL, "bits must be 2, 3 or 4 (got %d)", bits);
    if (group == 256 && f.explains256)
        return fail(AMQ_ESHAPE, "%s: a group of 256 spans two 128-column blocks and its parameters would need columns of the next block", f.serves);
    if (group != 32 && group != 64 && group != 128 && !(group == 256 && f.has256)) return fail(AMQ_ESHAPE, "%s (got %d)", f.serves, group);
    if (N <= 0 || (N % 16) != 0) return fail(AMQ_ESHAPE, "need N %% 16 == 0 (got N=%d)", N);
    if (f.has256 && (K <= 0 || (K % group) != 0 || (K % 128) != 0))
        return fail(AMQ_ESHAPE, "need K %% 128 == 0 and group %d dividing K (got K=%d)", group, K);
    if (K <= 0 || (K % 128) != 0) return fail(AMQ_ESHAPE, "need K %% 128 == 0 (got K=%d)", K);
    if (T < 1) return fail(AMQ_ESHAPE, "need at least one row of activations (got T=%d)", T);
    return AMQ_OK;
}

static int check_workspace(const char* what, size_t need, size_t got) {
    if (got < need) return fail(AMQ_EINVAL, "%s workspace too small: need %zu bytes, got %zu", what, need, got);
    return AMQ_OK;
}

size_t amq_hqq_quantize_workspace_bytes(int N, int K, int group) {
    if (check_quantize_shape(QUANT_HQQ, 4, N, K, group) != AMQ_OK) return 0;
    return amq::hqq_workspace_bytes(N, K, group);
}

int amq_hqq_quantize_f16(const void* W, int N, int K, int bits, int group, int round_zero, void* W_q, void* scale, void* zero,
                         void* info, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(AMQ_HQQ_INFO_BYTES == amq::HQQ_INFO_BYTES, "info block");
    if (!W || !W_q || !scale || !zero || !info || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W & 7) != 0 || ((uintptr_t)workspace & 3) != 0 || ((uintptr_t)info & 3) != 0 || ((uintptr_t)W_q & 3) != 0)
        return fail(AMQ_EINVAL, "W must be 8-byte aligned, W_q, info and workspace 4-byte aligned");
    if (int rc = check_quantize_shape(QUANT_HQQ, bits, N, K, group)) return rc;
    if (int rc = check_workspace("quantize", amq::hqq_workspace_bytes(N, K, group), workspace_bytes)) return rc;
    return check_hip(amq::launch_hqq_quantize(W, N, K, bits, group, round_zero != 0, W_q, scale, zero, info, workspace, (hipStream_t)stream),
                     "hqq_quantize");
}

size_t amq_gptq_quantize_workspace_bytes(int N, int K, int group) {
    if (check_quantize_shape(QUANT_GPTQ, 4, N, K, group) != AMQ_OK) return 0;
    return amq::gptq_workspace_bytes(N, K);
}

int amq_gptq_quantize_f16(const void* W, const void* U, int N, int K, int bits, int group, void* W_q, void* scale, void* zero, void* row_loss,
                          void* info, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(AMQ_GPTQ_INFO_BYTES == amq::GPTQ_INFO_BYTES, "info block");
    if (!W || !U || !W_q || !scale || !zero || !row_loss || !info || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W & 15) != 0 || ((uintptr_t)U & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)W_q & 3) != 0 ||
        ((uintptr_t)row_loss & 3) != 0 || ((uintptr_t)info & 3) != 0)
        return fail(AMQ_EINVAL, "W, U and workspace must be 16-byte aligned, W_q, row_loss and info 4-byte aligned");
    if (int rc = check_quantize_shape(QUANT_GPTQ, bits, N, K, group)) return rc;
    if (int rc = check_workspace("GPTQ", amq::gptq_workspace_bytes(N, K), workspace_bytes)) return rc;
    return check_hip(amq::launch_gptq_quantize(W, U, N, K, bits, group, W_q, scale, zero, row_loss, info, workspace, (hipStream_t)stream),
                     "gptq_quantize");
}

size_t amq_gptq_quantize_static_workspace_bytes(int N, int K, int group) { return amq_gptq_quantize_workspace_bytes(N, K, group); }

int amq_gptq_quantize_static_f16(const void* W, const void* U_p, const void* perm, int N, int K, int bits, int group, void* W_q, void* scale,
                                 void* zero, void* row_loss, void* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!W || !U_p || !perm || !W_q || !scale || !zero || !row_loss || !info || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W & 15) != 0 || ((uintptr_t)U_p & 15) != 0 || ((uintptr_t)perm & 15) != 0 || ((uintptr_t)workspace & 15) != 0 ||
        ((uintptr_t)W_q & 3) != 0 || ((uintptr_t)row_loss & 3) != 0 || ((uintptr_t)info & 3) != 0)
        return fail(AMQ_EINVAL, "W, U_p, perm and workspace must be 16-byte aligned, W_q, row_loss and info 4-byte aligned");
    if (int rc = check_quantize_shape(QUANT_GPTQ, bits, N, K, group)) return rc;
    if (int rc = check_workspace("GPTQ", amq::gptq_workspace_bytes(N, K), workspace_bytes)) return rc;
    return check_hip(amq::launch_gptq_quantize_static(W, U_p, perm, N, K, bits, group, W_q, scale, zero, row_loss, info, workspace,
                                                      (hipStream_t)stream), "gptq_quantize_static");
}

// OWQ: groups of 128 only (AMQ's); the shape rules of the range search and of the solve, in the order the header documents
static int check_owq_shape(int bits, int N, int K, int group, int num) {
    if (bits != 2 && bits != 3 && bits != 4) return fail(AMQ_EINVAL, "bits must be 2, 3 or 4 (got %d)", bits);
    if (group != 128) return fail(AMQ_ESHAPE, "the OWQ kernels serve groups of 128 only (got %d)", group);
    if (N <= 0 || (N % 16) != 0) return fail(AMQ_ESHAPE, "need N %% 16 == 0 (got N=%d)", N);
    if (K <= 0 || (K % 128) != 0) return fail(AMQ_ESHAPE, "need K %% 128 == 0 (got K=%d)", K);
    if (num < 1 || num > amq::OWQ_MAX_NUM) return fail(AMQ_ESHAPE, "num (range candidates) must be 1..%d (got %d)", (int)amq::OWQ_MAX_NUM, num);
    return AMQ_OK;
}
static int check_owq_outliers(int K, int n_out) {
    if (n_out < 0 || (n_out % 2) != 0 || n_out >= K) return fail(AMQ_ESHAPE, "n_out must be even and in 0 .. K - 2 (got n_out=%d, K=%d)", n_out, K);
    return AMQ_OK;
}

int amq_owq_range_f16(const void* W, int N, int K, int col0, int L, int bits, int num, void* scale, void* zero, void* choice, void* score,
                      void* wq_err, void* info, void* stream) {
    static_assert(AMQ_OWQ_INFO_BYTES == amq::OWQ_INFO_BYTES, "info block");
    if (!W || !scale || !zero || !choice || !score || !info) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W & 1) != 0 || ((uintptr_t)scale & 1) != 0 || ((uintptr_t)zero & 1) != 0 || ((uintptr_t)choice & 3) != 0 ||
        ((uintptr_t)score & 3) != 0 || ((uintptr_t)wq_err & 3) != 0 || ((uintptr_t)info & 3) != 0)
        return fail(AMQ_EINVAL, "W, scale and zero must be 2-byte aligned, choice, score, wq_err and info 4-byte aligned");
    if (int rc = check_owq_shape(bits, N, K, 128, num)) return rc;
    if (col0 < 0 || L < 1 || col0 > K - L) return fail(AMQ_ESHAPE, "the segment col0=%d, L=%d does not lie inside K=%d", col0, L, K);
    if (L > amq::OWQ_RANGE_MAX_L) return fail(AMQ_ESHAPE, "a segment of L=%d does not fit LDS (at most %d)", L, (int)amq::OWQ_RANGE_MAX_L);
    if (wq_err && (col0 != 0 || L != K)) return fail(AMQ_ESHAPE, "wq_err goes with the whole-row search (col0 = 0, L = K)");
    return check_hip(amq::launch_owq_range(W, N, K, col0, L, bits, num, scale, zero, choice, score, wq_err, info, (hipStream_t)stream), "owq_range");
}

size_t amq_owq_quantize_workspace_bytes(int N, int K, int n_out, int group) {
    if (check_owq_shape(4, N, K, group, 1) != AMQ_OK || check_owq_outliers(K, n_out) != AMQ_OK) return 0;
    return amq::owq_workspace_bytes(N, K, n_out);
}

int amq_owq_quantize_f16(const void* W_p, const void* U_p, int N, int K, int n_out, int bits, int group, int num, void* W_q, void* scale,
                         void* zero, void* W_out, void* choice, void* row_loss, void* info, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (!W_p || !U_p || !W_q || !scale || !zero || !choice || !row_loss || !info || !workspace || (!W_out && n_out != 0))
        return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W_p & 15) != 0 || ((uintptr_t)U_p & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)W_q & 3) != 0 ||
        ((uintptr_t)W_out & 1) != 0 || ((uintptr_t)choice & 3) != 0 || ((uintptr_t)row_loss & 3) != 0 || ((uintptr_t)info & 3) != 0)
        return fail(AMQ_EINVAL, "W_p, U_p and workspace must be 16-byte aligned, W_q, choice, row_loss and info 4-byte, W_out 2-byte aligned");
    if (int rc = check_owq_shape(bits, N, K, group, num)) return rc;
    if (int rc = check_owq_outliers(K, n_out)) return rc;
    if (int rc = check_workspace("OWQ", amq::owq_workspace_bytes(N, K, n_out), workspace_bytes)) return rc;
    return check_hip(amq::launch_owq_quantize(W_p, U_p, N, K, n_out, bits, num, W_q, scale, zero, W_out, choice, row_loss, info, workspace,
                                              (hipStream_t)stream), "owq_quantize");
}

int amq_owq_gather_f16(const void* x, int M, int K, const void* perm, int Kp, void* xg, void* stream) {
    if (!x || !perm || !xg) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)x & 1) != 0 || ((uintptr_t)perm & 3) != 0 || ((uintptr_t)xg & 3) != 0)
        return fail(AMQ_EINVAL, "x must be 2-byte aligned, perm and xg 4-byte aligned");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    if (K <= 0 || Kp <= 0 || (Kp % 128) != 0) return fail(AMQ_ESHAPE, "need K > 0 and Kp %% 128 == 0 (got K=%d Kp=%d)", K, Kp);
    return check_hip(amq::launch_owq_gather(x, M, K, perm, Kp, xg, (hipStream_t)stream), "owq_gather");
}

int amq_owq_outlier_add_f16(const void* x, int M, int K, const void* out_ids, int n_out, const void* W_out, void* y, int N, void* stream) {
    if (!x || !out_ids || !W_out || !y) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)x & 1) != 0 || ((uintptr_t)out_ids & 3) != 0 || ((uintptr_t)W_out & 1) != 0 || ((uintptr_t)y & 1) != 0)
        return fail(AMQ_EINVAL, "x, W_out and y must be 2-byte aligned, out_ids 4-byte aligned");
    if (M < 1 || M > 65535) return fail(AMQ_ESHAPE, "M must be 1..65535 (got %d)", M);
    if (N <= 0 || K <= 0 || n_out < 1 || n_out >= K) return fail(AMQ_ESHAPE, "need N > 0 and 1 <= n_out < K (got N=%d K=%d n_out=%d)", N, K, n_out);
    return check_hip(amq::launch_owq_outlier_add(x, M, K, out_ids, n_out, W_out, y, N, (hipStream_t)stream), "owq_outlier_add");
}

int amq_owq_stage_f16(const void* x, int R, int K, int act, const void* gamma, float eps, const void* x2, const amq_owq_part* parts, int n_parts,
                      void* stream) {
    static_assert(AMQ_OWQ_MAX_PARTS == amq::OWQ_STAGE_PARTS, "parts");
    if (!x || !parts || (act == AMQ_OWQ_ACT_RMSNORM && !gamma) || (act == AMQ_OWQ_ACT_SILU_MUL && !x2)) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)x & 15) != 0 || (act == AMQ_OWQ_ACT_RMSNORM && ((uintptr_t)gamma & 15) != 0) ||
        (act == AMQ_OWQ_ACT_SILU_MUL && ((uintptr_t)x2 & 15) != 0))
        return fail(AMQ_EINVAL, "x, x2 and gamma must be 16-byte aligned");
    if (act != AMQ_OWQ_ACT_NONE && act != AMQ_OWQ_ACT_RMSNORM && act != AMQ_OWQ_ACT_SILU_MUL) return fail(AMQ_EINVAL, "unknown activation %d", act);
    if (n_parts < 1 || n_parts > AMQ_OWQ_MAX_PARTS) return fail(AMQ_ESHAPE, "n_parts must be 1..%d (got %d)", AMQ_OWQ_MAX_PARTS, n_parts);
    if (R < 1 || R > amq::OWQ_STAGE_ROWS) return fail(AMQ_ESHAPE, "R must be 1..%d (got %d)", (int)amq::OWQ_STAGE_ROWS, R);
    if (K <= 0 || (K % 128) != 0) return fail(AMQ_ESHAPE, "need K %% 128 == 0 (got K=%d)", K);
    amq::OwqStageLaunchPart lp[AMQ_OWQ_MAX_PARTS];
    for (int i = 0; i < n_parts; ++i) {
        const amq_owq_part& p = parts[i];
        if (!p.xg || (p.n_out != 0 && (!p.perm || !p.out_ids || !p.W_out || !p.y))) return fail(AMQ_EINVAL, "part %d: null pointer", i);
        if (((uintptr_t)p.xg & 3) != 0 ||
            (p.n_out != 0 && (((uintptr_t)p.perm & 3) != 0 || ((uintptr_t)p.out_ids & 3) != 0 || ((uintptr_t)p.W_out & 1) != 0 ||
                              ((uintptr_t)p.y & 1) != 0 || ((uintptr_t)p.residual & 1) != 0)))
            return fail(AMQ_EINVAL, "part %d: xg, perm and out_ids must be 4-byte aligned, W_out, y and residual 2-byte aligned", i);
        if (p.n_out < 0 || (p.n_out % 2) != 0 || p.n_out >= K)
            return fail(AMQ_ESHAPE, "part %d: n_out must be even and in 0 .. K - 2 (got n_out=%d, K=%d)", i, p.n_out, K);
        if (p.n_out != 0 && (p.Kp <= 0 || (p.Kp % 128) != 0)) return fail(AMQ_ESHAPE, "part %d: need Kp %% 128 == 0 (got Kp=%d)", i, p.Kp);
        if (p.n_out != 0 && p.N <= 0) return fail(AMQ_ESHAPE, "part %d: need N > 0 (got N=%d)", i, p.N);
        lp[i] = {p.perm, p.out_ids, p.W_out, p.xg, p.y, p.residual, p.N, p.n_out, p.Kp};
    }
    return check_hip(amq::launch_owq_stage(x, R, K, act, gamma, eps, x2, lp, n_parts, (hipStream_t)stream), "owq_stage");
}

size_t amq_awq_quantize_workspace_bytes(int N, int K, int group) {
    if (check_quantize_shape(QUANT_AWQ, 4, N, K, group) != AMQ_OK) return 0;
    return amq::awq_quantize_workspace_bytes(N, K);
}

int amq_awq_quantize_f16(const void* W, const void* col_scale, const void* hi, const void* lo, int N, int K, int bits, int group, void* W_q,
                         void* scale, void* zero, void* dense, void* info, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(AMQ_AWQ_INFO_BYTES == amq::AWQ_INFO_BYTES, "info block");
    if (!W || !info || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if ((hi == nullptr) != (lo == nullptr)) return fail(AMQ_EINVAL, "null pointer: hi and lo come together or not at all");
    if ((W_q == nullptr) != (scale == nullptr) || (W_q == nullptr) != (zero == nullptr))
        return fail(AMQ_EINVAL, "null pointer: W_q, scale and zero come together or not at all");
    if (!W_q && !dense) return fail(AMQ_EINVAL, "null pointer: neither Format A nor the dense matrix is asked for");
    if (((uintptr_t)W & 15) != 0 || ((uintptr_t)dense & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)col_scale & 3) != 0 ||
        ((uintptr_t)W_q & 3) != 0 || ((uintptr_t)info & 3) != 0 || ((uintptr_t)hi & 1) != 0 || ((uintptr_t)lo & 1) != 0 ||
        ((uintptr_t)scale & 1) != 0 || ((uintptr_t)zero & 1) != 0)
        return fail(AMQ_EINVAL, "W, dense and workspace must be 16-byte aligned, col_scale, W_q and info 4-byte, hi, lo, scale and zero 2-byte");
    if (int rc = check_quantize_shape(QUANT_AWQ, bits, N, K, group)) return rc;
    if (int rc = check_workspace("AWQ quantize", amq::awq_quantize_workspace_bytes(N, K), workspace_bytes)) return rc;
    return check_hip(amq::launch_awq_quantize(W, col_scale, hi, lo, N, K, bits, group, W_q, scale, zero, dense, info, workspace,
                                              (hipStream_t)stream), "awq_quantize");
}

size_t amq_awq_clip_workspace_bytes(int N, int K, int T, int group) {
    if (check_quantize_shape(QUANT_AWQ, 4, N, K, group, T) != AMQ_OK) return 0;
    return amq::awq_clip_workspace_bytes(N, K, group);
}

int amq_awq_clip_f16(const void* W, const void* X, int N, int K, int T, int bits, int group, void* hi, void* lo, void* best, void* err,
                     void* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!W || !X || !hi || !lo || !best || !err || !info || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (((uintptr_t)W & 15) != 0 || ((uintptr_t)X & 15) != 0 || ((uintptr_t)hi & 1) != 0 || ((uintptr_t)lo & 1) != 0 || ((uintptr_t)best & 3) != 0 ||
        ((uintptr_t)err & 3) != 0 || ((uintptr_t)info & 3) != 0 || ((uintptr_t)workspace & 3) != 0)
        return fail(AMQ_EINVAL, "W and X must be 16-byte aligned, best, err, info and workspace 4-byte, hi and lo 2-byte");
    if (int rc = check_quantize_shape(QUANT_AWQ, bits, N, K, group, T)) return rc;
    if (int rc = check_workspace("AWQ clip", amq::awq_clip_workspace_bytes(N, K, group), workspace_bytes)) return rc;
    return check_hip(amq::launch_awq_clip(W, X, N, K, T, bits, group, hi, lo, best, err, info, workspace, (hipStream_t)stream), "awq_clip");
}

int amq_dequantize_f16(int bits, int mode, const void* qn, const void* mn, int N, int K, int group, void* W, void* stream) {
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (int rc = check_mode(mode)) return rc;
    mode = kernel_mode(mode);
    if (!qn || !mn || !W) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_dequantize(bits, mode, qn, mn, N, K, W, (hipStream_t)stream, amq::meta_pairs(group)), "dequantize");
}

int amq_dequantize_hqq_f16(int bits, const void* W_q, const void* scale, const void* zero, int N, int K, int group,
                           void* W, void* stream) {
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (!W_q || !scale || !zero || !W) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_dequantize_hqq(bits, W_q, scale, zero, N, K, W, (hipStream_t)stream, group), "dequantize_hqq");
}

#ifndef AMQ_GEMV_DEFAULT_MATH
#define AMQ_GEMV_DEFAULT_MATH AMQ_MATH_EXACT
#endif
int amq_default_gemv_math(void) { return AMQ_GEMV_DEFAULT_MATH; }

/* ---- fp16 matmul entry points: one segment reader, one option reader, one packed-GEMM validator and one route plan.  What differs between the
   entry points of a family is its form constant ("Matmul entry points: what is checked"). */

// The segments of a grouped call.  all_groups: the kernels read the finer groups' pairs (else one pair per 128 columns: check_shape128);
// raw_mode: the GEMV kernel tells AMQ_MODE_FMA1 apart, the others take it as AMQ_MODE_FMA
struct SegForm { const char* who; bool all_groups, raw_mode; };
constexpr SegForm SEG_GEMV{"amq_gemv_grouped_f16", true, true};
constexpr SegForm SEG_SUMS{"amq_gemv_grouped_sums_f16", true, true};
constexpr SegForm SEG_XFRAG{"amq_gemm_xfrag_grouped_f16", false, false};

// every segment's stride before any segment's shape, mode and pointers; act_mask: the segments that store fp16(silu(y)) (amq_gemv_grouped_f16 only)
static int read_segments(const SegForm& f, const amq_segment* segs, int nseg, int M, int K, int group, int act_mask, amq::GemvSeg* out) {
    for (int i = 0; i < nseg; ++i)
        if (int rc = check_strides(seg_name(f.who, i), M, K, 0, segs[i].N, segs[i].y_stride, 8, 0)) return rc;
    for (int i = 0; i < nseg; ++i) {
        const amq_segment& s = segs[i];
        if (int rc = f.all_groups ? check_shape(s.bits, s.N, K, group) : check_shape128(s.bits, s.N, K, group, f.who)) return rc;
        if (int rc = check_mode(s.mode)) return rc;
        if (!s.qweight_native || !s.meta_native || !s.y) return fail(AMQ_EINVAL, "segment %d: null pointer", i);
        amq::GemvSeg& d = out[i];
        d.qweight = s.qweight_native; d.meta = s.meta_native; d.bias = s.bias; d.residual = s.residual; d.y = s.y;
        d.N = s.N; d.bits = s.bits; d.mode = f.raw_mode ? s.mode : kernel_mode(s.mode);
        d.y_stride = s.y_stride ? s.y_stride : s.N;
        d.act = (act_mask >> i) & 1;
        if (d.act && s.residual) return fail(AMQ_EINVAL, "segment %d: an activated output (opts.act_mask) takes no residual", i);
    }
    return AMQ_OK;
}

// The options of a GEMV launch as launch_gemv / gemv_route see them: NULL = all zero = defaults, the default math resolved, the generic marker
// taken out of depth (auto depth under the generic kernel: everything below sees 0), the GEMV_FLAG_* of math and dot
struct GemvOptions { amq_gemv_opts o; bool generic; int flags; };
static int read_gemv_opts(const amq_gemv_opts* opts, int nseg, GemvOptions* out) {
    amq_gemv_opts o{};
    if (opts) o = *opts;
    if (o.math < AMQ_MATH_DEFAULT || o.math > AMQ_MATH_EXACT)
        return fail(AMQ_EINVAL, "opts.math must be AMQ_MATH_DEFAULT, AMQ_MATH_EXACT, AMQ_MATH_GROUPSCALE or AMQ_MATH_LINEAR");
    if (o.math == AMQ_MATH_DEFAULT) o.math = amq_default_gemv_math();
    if (o.waves != 0 && o.waves != 4 && o.waves != 8 && o.waves != 16) return fail(AMQ_EINVAL, "opts.waves must be 0, 4, 8 or 16");
    if (o.depth != 0 && o.depth != 2 && o.depth != 4 && o.depth != AMQ_GEMV_DEPTH_GENERIC) return fail(AMQ_EINVAL, "opts.depth must be 0, 2, 4 or AMQ_GEMV_DEPTH_GENERIC");
    out->generic = o.depth == AMQ_GEMV_DEPTH_GENERIC;
    if (out->generic) o.depth = 0;
    if (o.rpt < 0 || o.rpt > 64) return fail(AMQ_EINVAL, "opts.rpt (row-tiles per workgroup) must be 0..64");
    if (o.act_mask < 0 || o.act_mask >= (1 << nseg)) return fail(AMQ_EINVAL, "opts.act_mask names segments 0..%d (got 0x%x)", nseg - 1, o.act_mask);
    out->o = o;
    out->flags = (o.dot ? amq::GEMV_FLAG_DOT : 0) | (o.math == AMQ_MATH_LINEAR ? amq::GEMV_FLAG_LINEAR : 0) | (o.math == AMQ_MATH_GROUPSCALE ? amq::GEMV_FLAG_GS : 0);
    return AMQ_OK;
}

int amq_gemv_grouped_f16(const amq_segment* segs, int nseg, const void* x, const void* x2, const void* gamma,
                         float eps, int prologue, int M, int K, int group, int x_stride, const amq_gemv_opts* opts,
                         void* stream) {
    if (!segs || nseg < 1 || nseg > AMQ_MAX_SEGMENTS) return fail(AMQ_EINVAL, "nseg must be 1..%d (got %d)", AMQ_MAX_SEGMENTS, nseg);
    if (!x) return fail(AMQ_EINVAL, "null x");
    if ((prologue < AMQ_PRO_NONE || prologue > AMQ_PRO_SILU_MUL) && prologue != AMQ_PRO_MUL) return fail(AMQ_EINVAL, "unknown prologue %d", prologue);
    if (prologue == AMQ_PRO_RMSNORM && !gamma) return fail(AMQ_EINVAL, "RMSNorm prologue needs gamma");
    if (prologue == AMQ_PRO_SILU_MUL && !x2) return fail(AMQ_EINVAL, "SiLU*mul prologue needs x2");
    if (prologue == AMQ_PRO_MUL && !x2) return fail(AMQ_EINVAL, "mul prologue needs x2");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    if (int rc = check_strides("amq_gemv_grouped_f16", M, K, x_stride, 0, 0, 8, 0)) return rc;
    GemvOptions g;
    if (int rc = read_gemv_opts(opts, nseg, &g)) return rc;
    const amq_gemv_opts& o = g.o;
    const int gp = amq::meta_pairs(group);
    // (the activated output and the prologue that multiplies it live in the group-128 kernels; finer groups keep AMQ_PRO_SILU_MUL)
    if ((o.act_mask || prologue == AMQ_PRO_MUL) && gp != 1)
        return fail(AMQ_ESHAPE, "opts.act_mask / AMQ_PRO_MUL: groups of 128 (and multiples) only (got %d); use AMQ_PRO_SILU_MUL", group);
    const bool plain_form = !o.dot && o.math != AMQ_MATH_LINEAR && o.depth != 4 && gp == 1 && o.waves != 4;
    // (rows staged in two K phases -- 7 - 8 rows of K = 11008 -- need dense x rows and no full-row statistic: launch_gemv makes the same decision)
    const bool whole_rows = prologue == AMQ_PRO_RMSNORM || (x_stride != 0 && x_stride != K);
    if (M > amq::GEMV_MAX_M || amq::gemv_min_lds_bytes(M, K, plain_form && o.waves == 0 && o.rpt == 0, whole_rows) > LDS_LIMIT)
        return fail(AMQ_ESHAPE, "M=%d rows of K=%d%s do not fit LDS for the GEMV path; use amq_gemm_f16", M, K, (x_stride != 0 && x_stride != K) ? " (strided x)" : "");
    amq::GemvArgs a{};
    if (int rc = read_segments(SEG_GEMV, segs, nseg, M, K, group, o.act_mask, a.seg)) return rc;
    a.nseg = nseg; a.M = M; a.K = K; a.x_stride = x_stride ? x_stride : K;
    a.x = x; a.x2 = x2; a.gamma = gamma; a.eps = eps; a.prologue = prologue;
    a.flags = g.flags;
    a.force_waves = o.waves;
    a.force_depth = o.depth;
    a.force_rpt = o.rpt;
    a.gp = gp;
    a.generic = g.generic;
    if (gp > 1 && (o.dot || o.math == AMQ_MATH_LINEAR || o.depth == 4))
        return fail(AMQ_EINVAL, "groups of %d: the GEMV kernel's default form only (opts.math = AMQ_MATH_EXACT, opts.dot = 0, opts.depth = 0 / 2)", group);
    return check_hip(amq::launch_gemv(a, (hipStream_t)stream), "gemv");
}

int amq_gemv_route(int prologue, int M, int K, int group, int nseg, const int* bits, const int* modes, const amq_gemv_opts* opts) {
    if (!bits || !modes || nseg < 1 || nseg > AMQ_MAX_SEGMENTS) return fail(AMQ_EINVAL, "nseg must be 1..%d (got %d), bits and modes non-null", AMQ_MAX_SEGMENTS, nseg);
    if (int rc = check_group(group)) return rc;
    GemvOptions g;
    if (int rc = read_gemv_opts(opts, nseg, &g)) return rc;
    int km[AMQ_MAX_SEGMENTS];
    for (int i = 0; i < nseg; ++i) km[i] = modes[i] == AMQ_MODE_HQQ ? (int)amq::MODE_HQQ : (int)amq::MODE_FMA;      // (one-rounding buffers are generic either way)
    return amq::gemv_route(prologue, M, K, amq::meta_pairs(group), nseg, bits, km, g.flags, g.o.waves, g.o.depth, g.o.rpt, g.generic);
}

int amq_gemv_segment_order(int nseg, const int* bits, int act_mask, int* order, int* act_mask_out) {
    if (!bits || !order || nseg < 1 || nseg > AMQ_MAX_SEGMENTS) return fail(AMQ_EINVAL, "nseg must be 1..%d (got %d), bits and order non-null", AMQ_MAX_SEGMENTS, nseg);
    const int m = amq::gemv_segment_order(nseg, bits, act_mask, order);
    if (act_mask_out) *act_mask_out = m;
    return AMQ_OK;
}

int amq_gemv_grouped_sums_f16(const amq_segment* segs, int nseg, const void* x, const void* gamma, float eps, const float* sums_in,
                              float* sums_out, int M, int K, int group, void* stream) {
    if (!segs || nseg < 1 || nseg > AMQ_MAX_SEGMENTS) return fail(AMQ_EINVAL, "nseg must be 1..%d (got %d)", AMQ_MAX_SEGMENTS, nseg);
    if (!x) return fail(AMQ_EINVAL, "null x");
    if ((sums_in != nullptr) != (gamma != nullptr)) return fail(AMQ_EINVAL, "sums_in (the partial sums of squares of x) and gamma go together");
    if (M < 2 || M > 8) return fail(AMQ_ESHAPE, "the partial-sum forms live in the 2 .. 8-row kernels (got M=%d); one row: amq_gemv_grouped_f16 with AMQ_PRO_RMSNORM", M);
    if (amq::meta_pairs(group) != 1) return fail(AMQ_ESHAPE, "groups of 128 (and multiples) only (got %d)", group);
    if (K < 2048) return fail(AMQ_ESHAPE, "K >= 2048 (the 2 .. 8-row kernels run 8 or 16 waves per workgroup; got K=%d)", K);
    if (sums_out && nseg != 1) return fail(AMQ_EINVAL, "sums_out describes ONE output: nseg must be 1");
    if (sums_out && sums_in) return fail(AMQ_EINVAL, "sums_out is written by launches without a prologue (o_proj, down_proj): not together with sums_in");
    if (sums_in && K > 8192) return fail(AMQ_ESHAPE, "sums_in: K <= 8192 (K / 16 <= 512 partials per row; got K=%d)", K);
    const bool phased = amq::gemv_rows_phased(M, K, true, sums_in != nullptr);
    if (sums_in && phased) return fail(AMQ_ESHAPE, "M=%d rows of K=%d are staged in two K phases: no fused norm there", M, K);
    if (amq::gemv_min_lds_bytes(M, K, true, sums_in != nullptr) > LDS_LIMIT)
        return fail(AMQ_ESHAPE, "M=%d rows of K=%d do not fit LDS for the GEMV path", M, K);
    amq::GemvArgs a{};
    if (int rc = read_segments(SEG_SUMS, segs, nseg, M, K, group, 0, a.seg)) return rc;
    a.nseg = nseg; a.M = M; a.K = K; a.x_stride = K;
    a.x = x; a.x2 = nullptr; a.gamma = gamma; a.eps = eps;
    a.prologue = sums_in ? amq::PRO_RMSNORM_SUMS : amq::PRO_NONE;
    a.sums_in = sums_in; a.sums_out = sums_out;
    a.gp = 1;
    return check_hip(amq::launch_gemv(a, (hipStream_t)stream), "gemv_sums");
}

int amq_gemv_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, void* y,
                 int M, int N, int K, int group, int x_stride, int y_stride, void* stream) {
    amq_segment s{};
    s.qweight_native = qn; s.meta_native = mn; s.bias = bias; s.residual = nullptr; s.y = y;
    s.N = N; s.bits = bits; s.mode = mode; s.y_stride = y_stride;
    return amq_gemv_grouped_f16(&s, 1, x, nullptr, nullptr, 0.f, AMQ_PRO_NONE, M, K, group, x_stride, nullptr, stream);
}

// What a packed-GEMM call runs, derived here and nowhere else: dequantize-once or a fused kernel, the route the split-K policy is asked with (groups of
// 64 / 32 beyond their few-row kernel: the tiled kernel), the splits, and the bytes a workspace must hold -- the dequantized fp16 weights or the
// split-K partials, never both.  Without a workspace the call is a single pass through a fused kernel (splits = 1).  Outside the queries' domain: no workspace.
struct GemmPlan { bool deq; int sroute, splits; size_t need_bytes; };
static GemmPlan plan_gemm(int route, int M, int N, int K, int group, bool have_workspace) {
    if (M < 1 || N < 1 || K < 128 || route < AMQ_GEMM_AUTO || route > AMQ_GEMM_DEQ) return {false, route, 1, 0};
    const bool fine = group == 64 || group == 32;
    // few rows of fine groups: the pair-aware few-row kernel; then the tiled kernel; launches that fill 256 x 256 tiles: dequantize-once
    const bool deq = route == AMQ_GEMM_DEQ || (route == AMQ_GEMM_AUTO && (fine ? amq::gemm_fine_takes_deq(M, N, K) : amq::gemm_takes_deq(M, N, K)));
    const int sroute = fine && route == AMQ_GEMM_AUTO ? (int)AMQ_GEMM_TILED : route;
    if (deq) return {true, sroute, 1, (size_t)N * (size_t)K * 2};
    if (fine && amq::gemm_fine_takes_skinny(M)) return {false, sroute, 1, 0};          // (their few-row kernel takes no workspace)
    const int s = amq::gemm_pick_splits(M, N, K, sroute);
    if (s <= 1) return {false, sroute, 1, 0};
    return {false, sroute, have_workspace ? s : 1, (size_t)s * (size_t)M * (size_t)N * sizeof(float)};
}
// the launcher's arguments of a planned call; `workspace` is only looked at where the plan has a use for it
static amq::GemmArgs planned_args(const GemmPlan& p, const void* x, const void* qn, const void* mn, const void* bias, void* y, int M, int N, int K, int bits,
                                  int mode, int x_stride, int y_stride, const void* residual, const void* gate, void* workspace, int group) {
    return {x, qn, mn, bias, y, M, N, K, bits, mode, x_stride ? x_stride : K, y_stride ? y_stride : N, p.splits > 1 ? (float*)workspace : nullptr, p.splits,
            residual, gate, p.deq ? workspace : nullptr, amq::meta_pairs(group)};
}

size_t amq_gemm_splitk_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 128) return 0;
    const int s = amq::gemm_pick_splits(M, N, K);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)N * sizeof(float) : 0;
}
size_t amq_gemm_route_workspace_bytes_g(int route, int M, int N, int K, int group) { return plan_gemm(route, M, N, K, group, false).need_bytes; }
size_t amq_gemm_route_workspace_bytes(int route, int M, int N, int K) { return amq_gemm_route_workspace_bytes_g(route, M, N, K, 128); }

int amq_gemm_gated_fused_g(int route, int M, int N, int K, int use_workspace, int group) {
    if (M < 1 || N < 16 || K < 128 || route < AMQ_GEMM_AUTO || route > AMQ_GEMM_DEQ) return 0;
    static char present;       // (gemm_gate_fused only tests the workspace for presence; asking it without one needs a launcher change)
    const GemmPlan p = plan_gemm(route, M, N, K, group, use_workspace != 0);
    return amq::gemm_gate_fused(planned_args(p, nullptr, nullptr, nullptr, nullptr, nullptr, M, N, K, 4, AMQ_MODE_HQQ, 0, 0, nullptr, nullptr,
                                             use_workspace ? &present : nullptr, group > 0 ? group : 128), route) ? 1 : 0;
}
int amq_gemm_gated_fused(int route, int M, int N, int K, int use_workspace) { return amq_gemm_gated_fused_g(route, M, N, K, use_workspace, 128); }

// The packed-GEMM entry points.  ws: no workspace argument / the split-K entry point's (required, sized by amq_gemm_splitk_workspace_bytes) / the
// route family's (optional, sized by the plan).  gated: `other` is the gate (required, applied to the result) instead of the residual, and may
// alias y only where a kernel applies it.  deq_refusal: how the entry point words what the fp16-weight GEMM of the dequantize-once route cannot
// address (none: the entry point never runs it); deq_forced: a forced AMQ_GEMM_DEQ over groups of 128 is held to it too.
enum { WS_ABSENT, WS_SPLITK, WS_ROUTE };
struct GemmForm { const char* who; const char* what; int ws; bool gated; const char* deq_refusal; bool deq_forced; };
constexpr GemmForm GEMM_PLAIN{"amq_gemm_f16", "gemm", WS_ABSENT, false, nullptr, false};
constexpr GemmForm GEMM_SPLITK{"amq_gemm_splitk_f16", "gemm_splitk", WS_SPLITK, false, nullptr, false};
constexpr GemmForm GEMM_ROUTE{"amq_gemm_route_f16", "gemm", WS_ROUTE, false,
                              "AMQ_GEMM_DEQ: strides must be multiples of 8 (x) / 4 (y) halves and x, W must each span < 4 GiB", true};
constexpr GemmForm GEMM_GATED{"amq_gemm_gated_f16", "gemm_gated", WS_ROUTE, true,
                              "groups of %d (dequantize-once route): x_stride must be a multiple of 8 halves, N of 4, x and W must each span < 4 GiB", false};

static int gemm_call(const GemmForm& f, int route, int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, const void* other,
                     void* y, int M, int N, int K, int group, int x_stride, int y_stride, void* workspace, size_t workspace_bytes, void* stream,
                     amq::GemmNorm* norm = nullptr) {
    if (route < AMQ_GEMM_AUTO || route > AMQ_GEMM_DEQ) return fail(AMQ_EINVAL, "unknown GEMM route %d", route);
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (int rc = check_mode(mode)) return rc;
    if (int rc = check_strides(f.who, M, K, x_stride, N, y_stride, 8, fewrow_rows_of(route))) return rc;
    if (!x || !qn || !mn || !y || (f.gated && !other)) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    const bool fine = group == 64 || group == 32;
    // groups of 64 / 32 on a route call: the few-row kernel (AUTO / SKINNY) up to gemm_fine_takes_skinny rows, the tiled kernel (AUTO / TILED) or
    // dequantize-once (AUTO where it fills the chip, given the workspace; DEQ) beyond; the ring / wave-specialised kernels read one pair per tile
    if (route == AMQ_GEMM_SKINNY && M > 64 && !(fine && amq::gemm_fine_takes_skinny(M)))
        return fail(AMQ_ESHAPE, "the few-row kernel takes at most 64 rows (got %d)", M);
    if (fine && (route == AMQ_GEMM_RING || route == AMQ_GEMM_RING128 || route == AMQ_GEMM_WS))
        return fail(AMQ_EINVAL, "groups of %d: the ring / wave-specialised kernels read one (scale, zero) per 128 columns (use AMQ_GEMM_AUTO, _SKINNY, _TILED or the dequantize-once route _DEQ)", group);
    if (route == AMQ_GEMM_DEQ && !workspace) return fail(AMQ_EINVAL, "AMQ_GEMM_DEQ needs a workspace of N * K * 2 bytes for the fp16 weights");
    GemmPlan p{false, route, 1, 0};                        // (no workspace argument: a single pass through a fused kernel)
    if (f.ws == WS_SPLITK) p = {false, route, amq::gemm_pick_splits(M, N, K), amq_gemm_splitk_workspace_bytes(M, N, K)};
    if (f.ws == WS_ROUTE) p = plan_gemm(route, M, N, K, group, workspace != nullptr);
    if (workspace ? workspace_bytes < p.need_bytes : f.ws == WS_SPLITK)          // (the split-K entry point answers a missing workspace the same way)
        return fail(AMQ_EINVAL, "%sworkspace too small: need %zu bytes, got %zu", f.ws == WS_SPLITK ? "split-K " : "", p.need_bytes, workspace_bytes);
    const amq::GemmArgs a = planned_args(p, x, qn, mn, bias, y, M, N, K, bits, kernel_mode(mode), x_stride, y_stride, f.gated ? nullptr : other,
                                         f.gated ? other : nullptr, workspace, group);
    if (f.deq_refusal && ((f.deq_forced && route == AMQ_GEMM_DEQ) || (fine && p.deq)) && !amq::gemm_f16w_ok(M, N, K, a.x_stride, a.y_stride))
        return fail(AMQ_ESHAPE, f.deq_refusal, group);
    if (f.gated && other == y && !amq::gemm_gate_fused(a, route))
        return fail(AMQ_EINVAL, "gate may alias y only where the kernel applies it in its epilogue (amq_gemm_gated_fused)");
    return check_hip(amq::launch_gemm(a, (hipStream_t)stream, route, norm), f.what);
}

int amq_gemm_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, void* y,
                 int M, int N, int K, int group, int x_stride, int y_stride, void* stream) {
    // (groups of 64 / 32: the few-row or the tiled kernel -- no workspace here, so never dequantize-once)
    return gemm_call(GEMM_PLAIN, AMQ_GEMM_AUTO, bits, mode, x, qn, mn, bias, nullptr, y, M, N, K, group, x_stride, y_stride, nullptr, 0, stream);
}

int amq_gemm_splitk_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, void* y,
                        int M, int N, int K, int group, int x_stride, int y_stride, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (amq_gemm_splitk_workspace_bytes(M, N, K) == 0) return amq_gemm_f16(bits, mode, x, qn, mn, bias, y, M, N, K, group, x_stride, y_stride, stream);
    return gemm_call(GEMM_SPLITK, AMQ_GEMM_AUTO, bits, mode, x, qn, mn, bias, nullptr, y, M, N, K, group, x_stride, y_stride, workspace, workspace_bytes, stream);
}

int amq_gemm_route_f16(int route, int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias,
                       const void* residual, void* y, int M, int N, int K, int group, int x_stride, int y_stride,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return gemm_call(GEMM_ROUTE, route, bits, mode, x, qn, mn, bias, residual, y, M, N, K, group, x_stride, y_stride, workspace, workspace_bytes, stream);
}

int amq_gemm_res_norm_xfrag_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, const void* residual,
                                void* y, int M, int N, int K, int group, int x_stride, void* workspace, size_t workspace_bytes,
                                const void* gamma, float eps, void* xf, void* stream) {
    if (!gamma || !xf) return fail(AMQ_EINVAL, "null pointer");
    if (N < 128 || (N % 128) != 0) return fail(AMQ_ESHAPE, "the normed rows are handed on in fragment order: N %% 128 == 0 (got N=%d)", N);
    amq::GemmNorm norm{gamma, eps, xf, false};
    return gemm_call(GEMM_ROUTE, AMQ_GEMM_AUTO, bits, mode, x, qn, mn, bias, residual, y, M, N, K, group, x_stride, 0, workspace, workspace_bytes, stream, &norm);
}

int amq_gemm_gated_f16(int route, int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias,
                       const void* gate, void* y, int M, int N, int K, int group, int x_stride, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return gemm_call(GEMM_GATED, route, bits, mode, x, qn, mn, bias, gate, y, M, N, K, group, x_stride, 0, workspace, workspace_bytes, stream);
}

int amq_gemm_f16w_f16(const void* x, const void* w, const void* bias, const void* residual, const void* gate, void* y,
                      int M, int N, int K, int x_stride, int y_stride, void* stream) {
    if (!x || !w || !y) return fail(AMQ_EINVAL, "null pointer");
    if (residual && gate) return fail(AMQ_EINVAL, "residual and gate are exclusive");
    if (int rc = check_strides("amq_gemm_f16w_f16", M, K, x_stride, N, y_stride, 4, 0)) return rc;
    const int xs = x_stride ? x_stride : K, ys = y_stride ? y_stride : N;
    if (!amq::gemm_f16w_ok(M, N, K, xs, ys))
        return fail(AMQ_ESHAPE, "need M >= 1, N %% 16 == 0, K %% 128 == 0, x_stride %% 8 == 0, y_stride %% 4 == 0, x and W < 4 GiB each (got M=%d N=%d K=%d)", M, N, K);
    return check_hip(amq::launch_gemm_f16w(x, w, bias, residual, gate, y, M, N, K, xs, ys, (hipStream_t)stream), "gemm_f16w");
}

int amq_gemm_res_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, const void* residual,
                     void* y, int M, int N, int K, int group, int x_stride, int y_stride, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return amq_gemm_route_f16(AMQ_GEMM_AUTO, bits, mode, x, qn, mn, bias, residual, y, M, N, K, group, x_stride, y_stride,
                              workspace, workspace_bytes, stream);
}

size_t amq_xfrag_bytes(int M, int K) {
    if (M < 1 || K < 128 || (K % 128) != 0) return 0;
    return (size_t)((M + 63) / 64) * 64 * (size_t)K * 2;
}

int amq_xfrag_f16(const void* src, void* xf, int M, int K, long long stride_m, long long stride_kt, void* stream) {
    if (!src || !xf) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1 || K < 128 || (K % 128) != 0) return fail(AMQ_ESHAPE, "need M >= 1 and K %% 128 == 0 (got M=%d K=%d)", M, K);
    if (stride_m < 0 || stride_kt < 128 || (stride_m % 8) != 0 || (stride_kt % 8) != 0)
        return fail(AMQ_ESHAPE, "strides must be multiples of 8 halves, stride_kt >= 128");
    return check_hip(amq::launch_xfrag(src, xf, M, K, (long)stride_m, (long)stride_kt, (hipStream_t)stream), "xfrag");
}

int amq_rmsnorm_xfrag_f16(const void* x, const void* gamma, void* xf, int M, int K, float eps, void* stream) {
    if (!x || !gamma || !xf) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1 || K < 128 || (K % 128) != 0) return fail(AMQ_ESHAPE, "need M >= 1 and K %% 128 == 0 (got M=%d K=%d)", M, K);
    return check_hip(amq::launch_rmsnorm_xfrag(x, gamma, xf, M, K, eps, (hipStream_t)stream), "rmsnorm_xfrag");
}

int amq_gemm_xfrag_f16(int bits, int mode, const void* xf, const void* qn, const void* mn, const void* bias,
                       const void* gate, const void* residual, void* y, int M, int N, int K, int group, int y_stride,
                       void* stream) {
    if (int rc = check_shape128(bits, N, K, group, "amq_gemm_xfrag_f16")) return rc;
    if (int rc = check_mode(mode)) return rc;
    mode = kernel_mode(mode);
    if (int rc = check_strides("amq_gemm_xfrag_f16", M, K, 0, N, y_stride, 8, 0)) return rc;
    if (!xf || !qn || !mn || !y) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    if ((M + 63) / 64 > 65535) return fail(AMQ_ESHAPE, "M=%d exceeds one launch", M);
    amq::GemmArgs a{xf, qn, mn, bias, y, M, N, K, bits, mode, K, y_stride ? y_stride : N, nullptr, 1, residual, gate};
    return check_hip(amq::launch_gemm_xfrag(a, (hipStream_t)stream), "gemm_xfrag");
}

int amq_gemm_xfrag_grouped_f16(const amq_segment* segs, int nseg, const void* xf, int M, int K, int group, void* stream) {
    return amq_gemm_xfrag_grouped_form_f16(segs, nseg, xf, M, K, group, AMQ_FEWROW_AUTO, 0, stream);
}

int amq_gemm_xfrag_grouped_form_f16(const amq_segment* segs, int nseg, const void* xf, int M, int K, int group, int form, int blocks_per_wg,
                                    void* stream) {
    if (form < AMQ_FEWROW_AUTO || form > AMQ_FEWROW_STREAM) return fail(AMQ_EINVAL, "unknown few-row form %d", form);
    if (blocks_per_wg != 0 && (form != AMQ_FEWROW_STREAM || blocks_per_wg < 1 || blocks_per_wg > 6 || blocks_per_wg == 5))
        return fail(AMQ_EINVAL, "blocks_per_wg is 0, or 1 / 2 / 3 / 4 / 6 with AMQ_FEWROW_STREAM (got %d)", blocks_per_wg);
    if (!segs || nseg < 1 || nseg > AMQ_MAX_SEGMENTS) return fail(AMQ_EINVAL, "nseg must be 1..%d (got %d)", AMQ_MAX_SEGMENTS, nseg);
    if (!xf) return fail(AMQ_EINVAL, "null xf");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    if ((M + 63) / 64 > 65535) return fail(AMQ_ESHAPE, "M=%d exceeds one launch", M);
    amq::GemvSeg gs[AMQ_MAX_SEGMENTS] = {};
    if (int rc = read_segments(SEG_XFRAG, segs, nseg, M, K, group, 0, gs)) return rc;
    return check_hip(amq::launch_gemm_xfrag_grouped(xf, M, K, gs, nseg, (hipStream_t)stream, form, blocks_per_wg), "gemm_xfrag_grouped");
}


#ifdef AMQ_AB_ROUTES     /* A/B routes: exported by libamq_hip_ab.so (make ab), declared in include/amq_hip_ab.h */
int amq_gemv_qkv_attn_f16(const amq_segment* segs, const void* x, const void* gamma, float eps, int K, int group, void* kcache,
                          void* vcache, void* out, const void* step_state, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                          void* tickets, void* stream) {
    if (!segs || !x || !gamma || !kcache || !vcache || !out || !step_state || !tickets) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (n_heads < 1 || n_kv_heads < 1 || (n_heads % n_kv_heads) != 0 || n_heads > 255) return fail(AMQ_ESHAPE, "bad head counts %d / %d", n_heads, n_kv_heads);
    if (K > 8192) return fail(AMQ_ESHAPE, "K = %d: the fused launch serves K <= 8192", K);
    if (max_seq < 1 || amq::gemv_qkv_attn_lds_bytes(K, max_seq) > LDS_LIMIT) return fail(AMQ_ESHAPE, "max_seq=%d too long for the single-pass decode attention", max_seq);
    const int Ns[3] = {n_heads * 128, n_kv_heads * 128, n_kv_heads * 128};
    amq::GemvArgs a{};
    for (int i = 0; i < 3; ++i) {
        const amq_segment& s = segs[i];
        if (int rc = check_shape128(s.bits, s.N, K, group, "amq_gemv_qkv_attn_f16")) return rc;
        if (int rc = check_mode(s.mode)) return rc;
        if (s.N != Ns[i]) return fail(AMQ_ESHAPE, "segment %d: N = %d, expected %d", i, s.N, Ns[i]);
        if (!s.qweight_native || !s.meta_native || !s.y) return fail(AMQ_EINVAL, "segment %d: null pointer", i);
        if (s.bias || s.residual) return fail(AMQ_EUNSUPPORTED, "segment %d: bias / residual are not part of the fused q/k/v + attention launch", i);
        amq::GemvSeg& d = a.seg[i];
        d.qweight = s.qweight_native; d.meta = s.meta_native; d.y = s.y; d.N = s.N; d.bits = s.bits; d.mode = kernel_mode(s.mode); d.y_stride = s.N;
    }
    a.nseg = 3; a.M = 1; a.K = K; a.x_stride = K; a.x = x; a.gamma = gamma; a.eps = eps; a.prologue = amq::PRO_RMSNORM;
    amq::AttnArgs t{segs[0].y, segs[1].y, segs[2].y, kcache, vcache, out, nullptr, 0, n_heads, n_kv_heads, max_seq, 10000.0f, nullptr, step_state};
    return check_hip(amq::launch_gemv_qkv_attn(a, t, (int*)tickets, (hipStream_t)stream), "gemv_qkv_attn");
}

size_t amq_decode_engine_image_bytes(int n_block) { return n_block > 0 ? amq::engine_image_bytes(n_block) : 0; }
size_t amq_decode_engine_scratch_bytes(int hidden, int inter, int n_kv_heads) {
    if (hidden < 1 || inter < 1 || n_kv_heads < 1) return 0;
    return amq::engine_scratch_bytes(hidden, inter, n_kv_heads);
}
size_t amq_decode_engine_sync_bytes(void) { return amq::engine_sync_bytes(); }

static int engine_shapes_ok(int hidden, int inter, int n_heads, int n_kv_heads, int head_dim) {
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (n_heads < 1 || n_kv_heads < 1 || (n_heads % n_kv_heads) != 0) return fail(AMQ_ESHAPE, "bad head counts %d / %d", n_heads, n_kv_heads);
    if (hidden != n_heads * 128) return fail(AMQ_ESHAPE, "hidden (%d) must equal n_heads * 128", hidden);
    if ((hidden % 128) != 0 || (inter % 128) != 0 || inter < 128) return fail(AMQ_ESHAPE, "hidden and inter must be multiples of 128");
    if (hidden > 32768 || inter > 32768) return fail(AMQ_ESHAPE, "hidden / inter above 32768 are not staged by the engine");
    return AMQ_OK;
}

int amq_decode_engine_image(const amq_engine_block* blocks, int n_block, int hidden, int inter, int n_heads, int n_kv_heads,
                            int head_dim, int group, void* image) {
    if (!blocks || !image || n_block < 1) return fail(AMQ_EINVAL, "null pointer / no blocks");
    if (int rc = engine_shapes_ok(hidden, inter, n_heads, n_kv_heads, head_dim)) return rc;
    const int kvd = n_kv_heads * 128;
    const int Ns[7] = {hidden, kvd, kvd, hidden, inter, inter, hidden};
    std::vector<amq::EngineLinearH> lin((size_t)n_block * 7);
    std::vector<const void*> ln1(n_block), ln2(n_block);
    std::vector<void*> kc(n_block), vc(n_block);
    for (int b = 0; b < n_block; ++b) {
        for (int i = 0; i < 7; ++i) {
            const amq_engine_linear& l = blocks[b].lin[i];
            const int K = i == 6 ? inter : hidden;
            if (l.N != Ns[i]) return fail(AMQ_ESHAPE, "block %d linear %d: N = %d, expected %d", b, i, l.N, Ns[i]);
            if (int rc = check_shape128(l.bits, l.N, K, group, "the decode engine")) return rc;
            if (int rc = check_mode(l.mode)) return rc;
            if (!l.qweight_native || !l.meta_native) return fail(AMQ_EINVAL, "block %d linear %d: null pointer", b, i);
            if (amq::native_qweight_bytes(l.bits, l.N, K) >= (1ull << 32)) return fail(AMQ_ESHAPE, "block %d linear %d spans 4 GiB or more", b, i);
            lin[(size_t)b * 7 + i] = amq::EngineLinearH{l.qweight_native, l.meta_native, l.N, l.bits, kernel_mode(l.mode)};
        }
        if (!blocks[b].ln1 || !blocks[b].ln2 || !blocks[b].kcache || !blocks[b].vcache) return fail(AMQ_EINVAL, "block %d: null pointer", b);
        ln1[b] = blocks[b].ln1; ln2[b] = blocks[b].ln2; kc[b] = blocks[b].kcache; vc[b] = blocks[b].vcache;
    }
    amq::engine_fill_image(image, n_block, lin.data(), ln1.data(), ln2.data(), kc.data(), vc.data(), hidden, inter);
    return AMQ_OK;
}

int amq_decode_engine_f16(const void* blocks_dev, int n_block, int hidden, int inter, int n_heads, int n_kv_heads, int head_dim,
                          int max_seq, float eps, void* x, void* scratch, size_t scratch_bytes, const void* step_state,
                          void* sync, size_t sync_bytes, int grid, void* stream) {
    if (!blocks_dev || !x || !scratch || !step_state || !sync) return fail(AMQ_EINVAL, "null pointer");
    if (n_block < 1) return fail(AMQ_EINVAL, "no blocks");
    if (int rc = engine_shapes_ok(hidden, inter, n_heads, n_kv_heads, head_dim)) return rc;
    if (max_seq < 1) return fail(AMQ_ESHAPE, "max_seq must be >= 1");
    if (grid < 0 || grid > 1024) return fail(AMQ_EINVAL, "grid must be 0 (one workgroup per CU) or 1..1024");
    if (scratch_bytes < amq::engine_scratch_bytes(hidden, inter, n_kv_heads))
        return fail(AMQ_EINVAL, "scratch too small: need %zu bytes, got %zu", amq::engine_scratch_bytes(hidden, inter, n_kv_heads), scratch_bytes);
    if (sync_bytes < amq::engine_sync_bytes()) return fail(AMQ_EINVAL, "sync workspace too small: need %zu bytes", amq::engine_sync_bytes());
    amq::EngineDesc d{};
    d.blocks_dev = blocks_dev; d.n_block = n_block; d.H = hidden; d.I = inter; d.n_heads = n_heads; d.n_kv_heads = n_kv_heads;
    d.max_seq = max_seq; d.eps = eps; d.x = x; d.scratch = scratch; d.state = step_state; d.sync = sync; d.grid = grid;
    amq::StreamDevice sd_((hipStream_t)stream);
    int cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail(AMQ_ELAUNCH, "no HIP device");
    const int P = grid > 0 ? grid : cus;
    if (P > cus) return fail(AMQ_EINVAL, "grid %d exceeds the %d CUs of the device: the workgroups must all be resident", P, cus);
    if (n_heads > P) return fail(AMQ_ESHAPE, "the attention stage needs one workgroup per head (%d heads, %d workgroups)", n_heads, P);
    if (amq::engine_lds_bytes(d, P) > LDS_LIMIT)
        return fail(AMQ_ESHAPE, "engine LDS need (%zu bytes: max_seq %d, hidden %d, inter %d) exceeds %zu", amq::engine_lds_bytes(d, P),
                    max_seq, hidden, inter, LDS_LIMIT);
    return check_hip(amq::launch_decode_engine(d, (hipStream_t)stream), "decode_engine");
}
#endif  // AMQ_AB_ROUTES

/* the q / k norm of the amq_*_qkn_f16 entry points: NULL = none (the entry point without the suffix); else both weights */
static int qk_norm_arg(const amq_qk_norm* norm, amq::QkNorm* out) {
    *out = amq::QkNorm{nullptr, nullptr, 0.f};
    if (!norm) return AMQ_OK;
    if (!norm->q_gamma || !norm->k_gamma) return fail(AMQ_EINVAL, "q / k norm: q_gamma and k_gamma go together (one of them is null)");
    if (!(norm->eps >= 0.f)) return fail(AMQ_EINVAL, "q / k norm: eps must be >= 0");
    *out = amq::QkNorm{norm->q_gamma, norm->k_gamma, norm->eps};
    return AMQ_OK;
}

int amq_rope_cache_f16(void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                       int rope_rows, int pos0, int S, int n_heads, int n_kv_heads, int head_dim, int max_seq, void* stream) {
    if (!q || !k || !v || !kcache || !vcache || !rope_table) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (S < 1 || n_heads < 1 || n_kv_heads < 1 || rope_rows < 1) return fail(AMQ_ESHAPE, "bad sizes");
    if (pos0 < 0 || pos0 + S > max_seq) return fail(AMQ_ESHAPE, "rows %d..%d do not fit the cache (max_seq %d)", pos0, pos0 + S, max_seq);

    return check_hip(amq::launch_rope_cache(q, k, v, kcache, vcache, rope_table, rope_rows, pos0, S, n_heads, n_kv_heads, max_seq,
                                            (hipStream_t)stream), "rope_cache");
}

int amq_rope_cache_batch_f16(void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                             int rope_rows, int pos0, int S, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                             void* stream) {
    return amq_rope_cache_qkn_f16(nullptr, q, k, v, kcache, vcache, rope_table, rope_rows, pos0, S, batch, n_heads, n_kv_heads, head_dim, max_seq, stream);
}

int amq_rope_cache_qkn_f16(const amq_qk_norm* norm, void* q, const void* k, const void* v, void* kcache, void* vcache, const void* rope_table,
                           int rope_rows, int pos0, int S, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                           void* stream) {
    amq::QkNorm nrm;
    if (int rc = qk_norm_arg(norm, &nrm)) return rc;
    if (!q || !k || !v || !kcache || !vcache || !rope_table) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (S < 1 || batch < 1 || n_heads < 1 || n_kv_heads < 1 || rope_rows < 1) return fail(AMQ_ESHAPE, "bad sizes");
    if (pos0 < 0 || pos0 + S > max_seq) return fail(AMQ_ESHAPE, "rows %d..%d do not fit the cache (max_seq %d)", pos0, pos0 + S, max_seq);
    if ((long long)S * batch * (n_heads + n_kv_heads) > (1ll << 36)) return fail(AMQ_ESHAPE, "too many rows for one launch");
    return check_hip(amq::launch_rope_cache(q, k, v, kcache, vcache, rope_table, rope_rows, pos0, S, n_heads, n_kv_heads, max_seq,
                                            (hipStream_t)stream, batch, norm ? &nrm : nullptr), "rope_cache_batch");
}

int amq_rope_rows_f16(void* q, void* k, const void* rope_table, int rope_rows, int pos0, int rows, int seq_len, int n_heads,
                      int n_kv_heads, int head_dim, void* stream) {
    return amq_rope_rows_qkn_f16(nullptr, q, k, rope_table, rope_rows, pos0, rows, seq_len, n_heads, n_kv_heads, head_dim, stream);
}

int amq_rope_rows_qkn_f16(const amq_qk_norm* norm, void* q, void* k, const void* rope_table, int rope_rows, int pos0, int rows, int seq_len,
                          int n_heads, int n_kv_heads, int head_dim, void* stream) {
    amq::QkNorm nrm;
    if (int rc = qk_norm_arg(norm, &nrm)) return rc;
    if (!q || !k || !rope_table) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (rows < 1 || seq_len < 1 || (rows % seq_len) != 0 || n_heads < 1 || n_kv_heads < 1 || rope_rows < 1 || pos0 < 0)
        return fail(AMQ_ESHAPE, "bad sizes (rows=%d must be a multiple of seq_len=%d)", rows, seq_len);
    if ((long long)rows * (n_heads + n_kv_heads) > (1ll << 36)) return fail(AMQ_ESHAPE, "rows=%d exceeds one launch", rows);
    return check_hip(amq::launch_rope_rows(q, k, rope_table, rope_rows, pos0, rows, seq_len, n_heads, n_kv_heads,
                                           (hipStream_t)stream, norm ? &nrm : nullptr), "rope_rows");
}

int amq_silu_mul_f16(const void* gate, const void* up, void* out, size_t n, void* stream) {
    if (!gate || !up || !out) return fail(AMQ_EINVAL, "null pointer");
    if (n == 0 || (n & 7)) return fail(AMQ_ESHAPE, "n must be a positive multiple of 8 (got %zu)", n);
    return check_hip(amq::launch_silu_mul(gate, up, out, (long)n, (hipStream_t)stream), "silu_mul");
}

int amq_linear_f16(int bits, int mode, const void* x, const void* qn, const void* mn, const void* bias, void* y,
                   int M, int N, int K, int group, void* stream) {
    // few rows: weight-streaming GEMV family; otherwise the tiled MFMA GEMM
    if (M <= 8 && amq::gemv_lds_bytes(M, K, 1) <= 64 * 1024)
        return amq_gemv_f16(bits, mode, x, qn, mn, bias, y, M, N, K, group, 0, 0, stream);
    if ((group == 64 || group == 32) && M <= amq::GEMV_MAX_M && amq::gemv_lds_bytes(M, K, 1) <= LDS_LIMIT)     // (more rows: amq_gemm_route_f16 + workspace)
        return amq_gemv_f16(bits, mode, x, qn, mn, bias, y, M, N, K, group, 0, 0, stream);
    return amq_gemm_f16(bits, mode, x, qn, mn, bias, y, M, N, K, group, 0, 0, stream);
}

// ---- bfloat16 variants (amq_bf16.hip) -------------------------------------------------------------------
int amq_dequantize_bf16(int bits, const void* qn, const void* mn, int N, int K, int group, void* W, void* stream) {
    if (int rc = check_shape128(bits, N, K, group, "amq_dequantize_bf16")) return rc;
    if (!qn || !mn || !W) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_dequantize_bf16(bits, qn, mn, N, K, W, (hipStream_t)stream), "dequantize_bf16");
}

int amq_dequantize_hqq_bf16(int bits, const void* W_q, const void* scale, const void* zero, int N, int K, int group, void* W, void* stream) {
    if (int rc = check_shape(bits, N, K, group)) return rc;
    if (!W_q || !scale || !zero || !W) return fail(AMQ_EINVAL, "null pointer");
    return check_hip(amq::launch_dequantize_hqq_bf16(bits, W_q, scale, zero, N, K, W, (hipStream_t)stream, group), "dequantize_hqq_bf16");
}

int amq_gemv_bf16(int bits, const void* x, const void* qn, const void* mn, const void* bias, const void* residual, void* y,
                  int M, int N, int K, int group, int x_stride, int y_stride, void* stream) {
    if (int rc = check_shape128(bits, N, K, group, "amq_gemv_bf16")) return rc;
    if (!x || !qn || !mn || !y) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1 || M > 16) return fail(AMQ_ESHAPE, "amq_gemv_bf16 takes 1 .. 16 rows (got %d); use amq_gemm_bf16", M);
    if (x_stride == 0) x_stride = K;
    if (y_stride == 0) y_stride = N;
    if (x_stride < K || y_stride < N) return fail(AMQ_ESHAPE, "row strides shorter than the rows (x_stride=%d K=%d y_stride=%d N=%d)", x_stride, K, y_stride, N);
    if (x_stride & 7) return fail(AMQ_ESHAPE, "amq_gemv_bf16 reads x in 16-byte pieces: x_stride must be a multiple of 8 elements (got %d)", x_stride);
    return check_hip(amq::launch_gemv_bf16(bits, x, qn, mn, bias, residual, y, M, N, K, x_stride, y_stride, (hipStream_t)stream), "gemv_bf16");
}

size_t amq_gemm_bf16_workspace_bytes(int M, int N, int K) {
    if (M <= 16 || N <= 0 || K <= 0) return 0;
    return (size_t)N * (size_t)K * 2;
}

int amq_gemm_bf16(int bits, const void* x, const void* qn, const void* mn, const void* bias, const void* residual, void* y,
                  int M, int N, int K, int group, int x_stride, int y_stride, void* workspace, size_t workspace_bytes, void* stream) {
    if (M >= 1 && M <= 16) return amq_gemv_bf16(bits, x, qn, mn, bias, residual, y, M, N, K, group, x_stride, y_stride, stream);
    if (int rc = check_shape128(bits, N, K, group, "amq_gemm_bf16")) return rc;
    if (!x || !qn || !mn || !y) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1) return fail(AMQ_ESHAPE, "M must be >= 1 (got %d)", M);
    if (x_stride == 0) x_stride = K;
    if (y_stride == 0) y_stride = N;
    if (x_stride < K || y_stride < N) return fail(AMQ_ESHAPE, "row strides shorter than the rows (x_stride=%d K=%d y_stride=%d N=%d)", x_stride, K, y_stride, N);
    const size_t need = amq_gemm_bf16_workspace_bytes(M, N, K);
    if (!workspace || workspace_bytes < need) return fail(AMQ_EINVAL, "amq_gemm_bf16 workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!amq::gemm_f16w_ok(M, N, K, x_stride, y_stride))
        return fail(AMQ_ESHAPE, "amq_gemm_bf16 beyond 16 rows needs x_stride %% 8 == 0, y_stride %% 4 == 0 and x, W spans below 4 GiB (M=%d N=%d K=%d)", M, N, K);
    if (int rc = check_hip(amq::launch_dequantize_bf16(bits, qn, mn, N, K, workspace, (hipStream_t)stream), "dequantize_bf16")) return rc;
    return check_hip(amq::launch_gemm_bf16w(x, workspace, bias, residual, y, M, N, K, x_stride, y_stride, (hipStream_t)stream), "gemm_bf16");
}

// ---- reference-FFI-shaped entry points ---------------------------------------------------------------
namespace {
struct CompatWs { void* qn; void* mn; void* ytmp; };
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
CompatWs carve(void* ws, int bits, int M, int N, int K) {
    char* p = (char*)ws;
    CompatWs c;
    c.qn = p; p += align256(amq::native_qweight_bytes(bits, N, K));
    c.mn = p; p += align256(amq::native_meta_bytes(N, K, 4));            // (room for the finest group the repack writes: 32)
    c.ytmp = p;
    (void)M;
    return c;
}
}  // namespace

size_t amq_compat_workspace_bytes(int bits, int M, int N, int K) {
    if (N <= 0 || K <= 0 || M <= 0) return 0;
    return align256(amq::native_qweight_bytes(bits, N, K)) + align256(amq::native_meta_bytes(N, K, 4)) + align256((size_t)M * N * 2);
}

int amq_vecquantmatmul_faster_old(int bits, const void* vec, const void* mat, void* mul, const void* scales,
                                  const void* zeros, int groupsize, int vec_height, int batch, int height, int width,
                                  void* workspace, size_t workspace_bytes, int workspace_valid, void* stream) {
    if (bits != 2 && bits != 3 && bits != 4) return fail(AMQ_EINVAL, "bits must be 2, 3 or 4 (got %d)", bits);
    if (height <= 0 || (height * 32) % bits) return fail(AMQ_ESHAPE, "mat height %d is not K/32*bits", height);
    const int K = height * 32 / bits, N = width, M = batch;
    if (int rc = check_shape(bits, N, K, groupsize)) return rc;
    if (vec_height != K / 2) return fail(AMQ_ESHAPE, "vec_height must be K/2 = %d (got %d)", K / 2, vec_height);
    if (!vec || !mat || !mul || !scales || !zeros || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1) return fail(AMQ_ESHAPE, "batch must be >= 1");
    if (workspace_bytes < amq_compat_workspace_bytes(bits, M, N, K)) return fail(AMQ_EINVAL, "workspace too small");
    const CompatWs w = carve(workspace, bits, M, N, K);
    if (!workspace_valid)
        if (int rc = amq_repack_from_gptq(bits, mat, scales, zeros, N, K, groupsize, w.qn, w.mn, stream)) return rc;
    if (int rc = amq_linear_f16(bits, AMQ_MODE_FMA, vec, w.qn, w.mn, nullptr, w.ytmp, M, N, K, groupsize, stream)) return rc;
    return check_hip(amq::launch_accumulate_f32(mul, w.ytmp, (size_t)M * N, (hipStream_t)stream), "accumulate");
}

static int compat_awq(const void* x, const void* kernel, const void* scales, const void* scaled_zeros, void* y,
                      int m, int n, int k, int group_size, void* workspace, size_t workspace_bytes, int workspace_valid,
                      void* stream, bool gemm) {
    if (int rc = check_shape(4, n, k, group_size)) return rc;
    if (!x || !kernel || !scales || !scaled_zeros || !y || !workspace) return fail(AMQ_EINVAL, "null pointer");
    if (m < 1) return fail(AMQ_ESHAPE, "m must be >= 1");
    if (workspace_bytes < amq_compat_workspace_bytes(4, 1, n, k)) return fail(AMQ_EINVAL, "workspace too small");
    const CompatWs w = carve(workspace, 4, 1, n, k);
    if (!workspace_valid)
        if (int rc = amq_repack_from_awq(kernel, scales, scaled_zeros, n, k, group_size, w.qn, w.mn, stream)) return rc;
    if (gemm) return amq_gemm_f16(4, AMQ_MODE_FMA, x, w.qn, w.mn, nullptr, y, m, n, k, group_size, 0, 0, stream);
    return amq_linear_f16(4, AMQ_MODE_FMA, x, w.qn, w.mn, nullptr, y, m, n, k, group_size, stream);
}

int amq_gemv_4bit(const void* x, const void* kernel, const void* scales, const void* scaled_zeros, void* y,
                  int m, int n, int k, int group_size, void* workspace, size_t workspace_bytes, int workspace_valid, void* stream) {
    return compat_awq(x, kernel, scales, scaled_zeros, y, m, n, k, group_size, workspace, workspace_bytes, workspace_valid, stream, false);
}

int amq_gemm_4bit(const void* x, const void* kernel, const void* scales, const void* scaled_zeros, void* y,
                  int m, int n, int k, int group_size, void* workspace, size_t workspace_bytes, int workspace_valid, void* stream) {
    return compat_awq(x, kernel, scales, scaled_zeros, y, m, n, k, group_size, workspace, workspace_bytes, workspace_valid, stream, true);
}

int amq_rmsnorm_f16(const void* x, const void* gamma, void* y, int M, int K, float eps, void* stream) {
    if (!x || !gamma || !y) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1 || K < 8 || (K % 8) != 0) return fail(AMQ_ESHAPE, "need M >= 1 and K %% 8 == 0 (got M=%d K=%d)", M, K);
    return check_hip(amq::launch_rmsnorm(x, gamma, y, M, K, eps, (hipStream_t)stream), "rmsnorm");
}

int amq_gemv_f16w(const void* x, const void* W, const void* bias, void* y, const void* gamma, float eps,
                  int N, int K, void* stream) {
    if (!x || !W || !y) return fail(AMQ_EINVAL, "null pointer");
    if (N < 1 || K < 8 || (K % 8) != 0) return fail(AMQ_ESHAPE, "need K %% 8 == 0 (got N=%d K=%d)", N, K);
    if ((size_t)K * 2 + 64 > 64 * 1024) return fail(AMQ_ESHAPE, "K=%d too large for the fp16-weight GEMV", K);
    return check_hip(amq::launch_gemv_f16w(x, W, bias, y, gamma, eps, N, K, (hipStream_t)stream), "gemv_f16w");
}

int amq_gemv_f16w_rows(const void* x, const void* W, const void* bias, void* y, const void* gamma, float eps, int M,
                       int N, int K, void* stream) {
    if (!x || !W || !y) return fail(AMQ_EINVAL, "null pointer");
    if (M < 1 || M > 8) return fail(AMQ_ESHAPE, "M must be 1..8 (got %d)", M);
    if (N < 1 || K < 8 || (K % 8) != 0) return fail(AMQ_ESHAPE, "need N >= 1 and K %% 8 == 0 (got %d, %d)", N, K);
    if ((size_t)M * K * 2 + 64 > LDS_LIMIT) return fail(AMQ_ESHAPE, "%d rows of K=%d do not fit LDS", M, K);
    return check_hip(amq::launch_gemv_f16w(x, W, bias, y, gamma, eps, N, K, (hipStream_t)stream, M), "gemv_f16w_rows");
}

/* ---- the 8-bit lm_head (amq_lm8.hip): what both entry points require of the layer, one rule per refusal ---- */
static int check_lm8(const char* who, int N, int K, int group) {
    if (group != 128) return fail(AMQ_ESHAPE, "%s: group must be 128 (got %d)", who, group);
    if (K < 128 || (K % 128) != 0) return fail(AMQ_ESHAPE, "%s: K must be a positive multiple of 128 (got %d)", who, K);
    if (N < 1) return fail(AMQ_ESHAPE, "%s: N must be >= 1 (got %d)", who, N);
    return AMQ_OK;
}
// the kernels move x, gamma, codes and the dequantized rows in 16-byte pieces and a (scale, zero) pair as one dword
static int check_lm8_aligned(const char* who, const char* name, const void* p, size_t align) {
    if (p && ((size_t)p % align) != 0) return fail(AMQ_EINVAL, "%s: %s must be %d-byte aligned", who, name, (int)align);
    return AMQ_OK;
}

int amq_lm8_gemv_f16(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K, int group,
                     void* stream) {
    const char* who = "amq_lm8_gemv_f16";
    if (!x || !codes || !meta || !y) return fail(AMQ_EINVAL, "%s: null pointer", who);
    if (int rc = check_lm8_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_lm8_aligned(who, "codes", codes, 16)) return rc;
    if (int rc = check_lm8_aligned(who, "meta", meta, 4)) return rc;
    if (int rc = check_lm8_aligned(who, "gamma", gamma, 16)) return rc;
    if (int rc = check_lm8_aligned(who, "y", y, 2)) return rc;
    if (M < 1 || M > 8) return fail(AMQ_ESHAPE, "%s: M must be 1..8 (got %d)", who, M);
    if (int rc = check_lm8(who, N, K, group)) return rc;
    if (amq::lm8_gemv_lds_bytes(M, K) > LDS_LIMIT) return fail(AMQ_ESHAPE, "%s: %d rows of K=%d do not fit LDS", who, M, K);
    return check_hip(amq::launch_lm8_gemv(x, codes, meta, y, gamma, eps, M, N, K, (hipStream_t)stream), "lm8_gemv");
}

int amq_lm8_dequantize_f16(const void* codes, const void* meta, void* out, int row0, int rows, int N, int K, int group, void* stream) {
    const char* who = "amq_lm8_dequantize_f16";
    if (!codes || !meta || !out) return fail(AMQ_EINVAL, "%s: null pointer", who);
    if (int rc = check_lm8_aligned(who, "codes", codes, 16)) return rc;
    if (int rc = check_lm8_aligned(who, "meta", meta, 4)) return rc;
    if (int rc = check_lm8_aligned(who, "out", out, 16)) return rc;
    if (int rc = check_lm8(who, N, K, group)) return rc;
    if (row0 < 0 || rows < 1 || rows > N - row0) return fail(AMQ_ESHAPE, "%s: rows %d .. %d + %d outside the layer's %d rows", who, row0, row0, rows, N);
    return check_hip(amq::launch_lm8_dequantize(codes, meta, out, row0, rows, K, (hipStream_t)stream), "lm8_dequantize");
}

/* ---- decode attention: ten entry points, one validator and dispatcher.  What differs between them is the AttnForm ("Decode-step
   entry points: what is checked"); the checks run in the order of this function for every one of them ---- */
enum : unsigned {           // where the position(s) of the new token(s) may come from
    POS_HOST = 1,           // the host int `pos`: checked against max_seq when neither of the next two is given
    POS_DEV = 2,            // the device int32 `pos_dev`
    POS_BLOCK = 4,          // one step-state block for the whole batch
    POS_BLOCKS = 8,         // an array of `batch` step-state blocks: every sequence at its own position
    POS_ROWS = 16,          // ... the blocks being consecutive positions of ONE sequence
};
enum AttnSplits { SPLITS_NONE, SPLITS_REQUIRED, SPLITS_OPTIONAL };      // n_splits: not an argument / 1..1024 / 0 (one workgroup per head) or 1..1024
struct AttnForm {
    unsigned pos;           // POS_*: without POS_HOST / POS_DEV the step state is a required pointer
    int batch_min, batch_max;
    AttnSplits splits;      // SPLITS_REQUIRED: workspace and tickets are required pointers too
    size_t extra_lds;       // bytes beside the score array and the kernel's own 6 * 128 + 17 KiB
    const char* what;       // names the launch in a HIP error
    const char* rows;       // what `batch` counts, in messages
    bool grouped = false;   // the matrix-core grouped-query kernels only: 2 <= n_heads / n_kv_heads <= 16, their fixed LDS, tickets unused
};
constexpr int NO_BOUND = 0x7fffffff;
constexpr AttnForm ATTN_POS{POS_HOST | POS_DEV, 1, NO_BOUND, SPLITS_NONE, 0, "attn_decode", "batch"};
constexpr AttnForm ATTN_CUR{POS_BLOCK, 1, NO_BOUND, SPLITS_NONE, 0, "attn_decode_cur", "batch"};
constexpr AttnForm ATTN_SPLIT{POS_HOST | POS_DEV | POS_BLOCK, 1, 65535, SPLITS_REQUIRED, 0, "attn_decode_split", "batch"};
constexpr AttnForm ATTN_SEQ{POS_BLOCKS, 1, 65535, SPLITS_OPTIONAL, 0, "attn_decode_seq", "batch"};
// (rows: the earlier rows' rotated keys and values sit behind the score array)
constexpr AttnForm ATTN_ROWS{POS_ROWS, 2, AMQ_LOOKUP_MAX_ROWS, SPLITS_OPTIONAL, 2 * 7 * 128 * 2 + 16, "attn_decode_rows", "rows"};
constexpr AttnForm ATTN_ROWS_GQA{POS_ROWS, 2, AMQ_LOOKUP_MAX_ROWS, SPLITS_REQUIRED, 0, "attn_decode_rows_gqa", "rows", true};

size_t amq_attn_decode_split_workspace_bytes(int batch, int n_heads, int n_splits) {
    if (batch < 1 || n_heads < 1 || n_splits < 1) return 0;
    return (size_t)batch * n_heads * n_splits * 132 * sizeof(float);
}

// An entry point passes what its signature lacks as: state / pos_dev / rope_table / workspace / tickets null, pos 0, rope_theta 10000, n_splits 0.
static int attn_decode(const AttnForm& f, const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                       const void* state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                       float rope_theta, const void* rope_table, int n_splits, void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    amq::QkNorm nrm;
    if (int rc = qk_norm_arg(norm, &nrm)) return rc;
    const bool state_required = !(f.pos & (POS_HOST | POS_DEV));
    if (!q || !k || !v || !kcache || !vcache || !out || (state_required && !state) || (f.splits == SPLITS_REQUIRED && (!workspace || !tickets)))
        return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (batch < f.batch_min || batch > f.batch_max) return fail(AMQ_ESHAPE, "%s must be %d..%d (got %d)", f.rows, f.batch_min, f.batch_max, batch);
    if (n_heads < 1 || n_heads > 255 || n_kv_heads < 1 || (n_heads % n_kv_heads) != 0)
        return fail(AMQ_ESHAPE, "bad head configuration (%d q heads, %d kv heads)", n_heads, n_kv_heads);
    if (f.grouped && (n_heads / n_kv_heads < 2 || n_heads / n_kv_heads > 16))
        return fail(AMQ_ESHAPE, "%s serves 2..16 query heads per kv head (got %d / %d)", f.what, n_heads, n_kv_heads);
    if (max_seq < 1 || (!state && !pos_dev && (pos < 0 || pos >= max_seq)))
        return fail(AMQ_ESHAPE, "position %d outside the cache (max_seq=%d)", pos, max_seq);
    if (f.grouped && max_seq > (1 << 24)) return fail(AMQ_ESHAPE, "%s forms a key's byte offset in 32 bits: max_seq <= 2^24 (got %d)", f.what, max_seq);
    if (f.splits != SPLITS_NONE && (n_splits < (f.splits == SPLITS_REQUIRED ? 1 : 0) || n_splits > 1024))
        return fail(AMQ_EINVAL, "n_splits must be %s1..1024 (got %d)", f.splits == SPLITS_REQUIRED ? "" : "0 (one workgroup per head) or ", n_splits);
    if (n_splits && (!workspace || !tickets)) return fail(AMQ_EINVAL, "null pointer (workspace / tickets are required with n_splits >= 1)");
    int keys = max_seq;             // ... one workgroup scores: the whole cache, or its chunk of it
    if (n_splits) {
        keys = (((max_seq + n_splits - 1) / n_splits) + 31) & ~31;
        keys = keys < amq::ATT_MIN_CHUNK ? amq::ATT_MIN_CHUNK : keys;
    }
    if (!f.grouped && 6 * 128 + (size_t)keys * 4 + f.extra_lds + 17 * 1024 > LDS_LIMIT)
        return n_splits ? fail(AMQ_ESHAPE, "max_seq=%d over %d splits leaves chunks of %d keys: too long", max_seq, n_splits, keys)
                        : fail(AMQ_ESHAPE, "max_seq=%d too long for the single-pass decode attention", max_seq);
    const size_t need = amq_attn_decode_split_workspace_bytes(batch, n_heads, n_splits);
    if (workspace_bytes < need) return fail(AMQ_EINVAL, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    // a step state carries the position and its cos/sin row: pos_dev, rope_theta and rope_table are then not looked at
    amq::AttnArgs a{q, k, v, kcache, vcache, out, state ? nullptr : pos_dev, pos, n_heads, n_kv_heads, max_seq, state ? 10000.0f : rope_theta,
                    state ? nullptr : rope_table, state, (f.pos & (POS_BLOCKS | POS_ROWS)) != 0, (f.pos & POS_ROWS) != 0};
    a.norm = nrm;
    const hipError_t e = f.grouped ? amq::launch_attn_decode_gqa_rows(a, batch, n_splits, workspace, (hipStream_t)stream)
                         : n_splits ? amq::launch_attn_decode_split(a, batch, n_splits, workspace, tickets, (hipStream_t)stream)
                                    : amq::launch_attn_decode(a, batch, (hipStream_t)stream);
    if (e == hipSuccess) return AMQ_OK;
    return fail(AMQ_ELAUNCH, "%s%s: %s", f.what, n_splits && f.splits == SPLITS_OPTIONAL ? " (split)" : "", hipGetErrorString(e));
}

int amq_attn_decode_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                        const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                        int max_seq, float rope_theta, const void* rope_table, void* stream) {
    return amq_attn_decode_qkn_f16(nullptr, q, k, v, kcache, vcache, out, pos_dev, pos, batch, n_heads, n_kv_heads, head_dim, max_seq, rope_theta, rope_table, stream);
}

int amq_attn_decode_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                            const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                            int max_seq, float rope_theta, const void* rope_table, void* stream) {
    return attn_decode(ATTN_POS, norm, q, k, v, kcache, vcache, out, nullptr, pos_dev, pos, batch, n_heads, n_kv_heads, head_dim, max_seq, rope_theta, rope_table,
                       0, nullptr, 0, nullptr, stream);
}

int amq_attn_decode_cur_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                            const void* step_state, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                            void* stream) {
    return amq_attn_decode_cur_qkn_f16(nullptr, q, k, v, kcache, vcache, out, step_state, batch, n_heads, n_kv_heads, head_dim, max_seq, stream);
}

int amq_attn_decode_cur_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                const void* step_state, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                void* stream) {
    return attn_decode(ATTN_CUR, norm, q, k, v, kcache, vcache, out, step_state, nullptr, 0, batch, n_heads, n_kv_heads, head_dim, max_seq, 10000.0f, nullptr,
                       0, nullptr, 0, nullptr, stream);
}

int amq_attn_decode_split_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                              const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads,
                              int head_dim, int max_seq, float rope_theta, const void* rope_table, int n_splits,
                              void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    return amq_attn_decode_split_qkn_f16(nullptr, q, k, v, kcache, vcache, out, step_state, pos_dev, pos, batch, n_heads, n_kv_heads, head_dim, max_seq, rope_theta, rope_table, n_splits,
                                         workspace, workspace_bytes, tickets, stream);
}

int amq_attn_decode_split_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                  const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads,
                                  int head_dim, int max_seq, float rope_theta, const void* rope_table, int n_splits,
                                  void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    return attn_decode(ATTN_SPLIT, norm, q, k, v, kcache, vcache, out, step_state, pos_dev, pos, batch, n_heads, n_kv_heads, head_dim, max_seq, rope_theta, rope_table,
                       n_splits, workspace, workspace_bytes, tickets, stream);
}

/* ---- 8-bit KV cache (amq_attn_kv8.hip) ---- */
int amq_kv8_store_f16(const void* k, const void* v, void* kc8, void* ks, void* vc8, void* vs, int pos0, int S, int batch, int n_kv_heads,
                      int head_dim, int max_seq, void* stream) {
    if (!k || !v || !kc8 || !ks || !vc8 || !vs) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (batch < 1 || S < 1 || n_kv_heads < 1 || n_kv_heads > 255) return fail(AMQ_ESHAPE, "need batch, S >= 1 and 1..255 kv heads (got %d, %d, %d)", batch, S, n_kv_heads);
    if (max_seq < 1 || pos0 < 0 || (long long)pos0 + S > max_seq)
        return fail(AMQ_ESHAPE, "rows %d .. %lld outside the cache (max_seq=%d)", pos0, (long long)pos0 + S - 1, max_seq);
    return check_hip(amq::launch_kv8_store(k, v, kc8, ks, vc8, vs, pos0, S, batch, n_kv_heads, max_seq, (hipStream_t)stream), "kv8_store");
}

size_t amq_attn_decode_kv8_workspace_bytes(int batch, int n_heads, int n_splits) {
    if (batch < 1 || n_heads < 1 || n_splits < 1) return 0;
    return (size_t)batch * n_heads * n_splits * 132 * sizeof(float);
}

int amq_attn_decode_kv8_f16(const void* q, const void* k, const void* v, void* kc8, void* ks, void* vc8, void* vs, void* out,
                            const void* step_state, const int* pos_dev, int pos, int batch, int n_heads, int n_kv_heads, int head_dim,
                            int max_seq, float rope_theta, const void* rope_table, int n_splits, void* workspace, size_t workspace_bytes,
                            void* tickets, void* stream) {
    if (!q || !k || !v || !kc8 || !ks || !vc8 || !vs || !out || !workspace || !tickets) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (batch < 1 || batch > 65535) return fail(AMQ_ESHAPE, "batch must be 1..65535 (got %d)", batch);
    if (n_heads < 1 || n_heads > 255 || n_kv_heads < 1 || (n_heads % n_kv_heads) != 0 || n_heads / n_kv_heads > 16)
        return fail(AMQ_ESHAPE, "bad head configuration (%d q heads, %d kv heads; 1..16 query heads per kv head)", n_heads, n_kv_heads);
    if (max_seq < 1 || (!step_state && !pos_dev && (pos < 0 || pos >= max_seq)))
        return fail(AMQ_ESHAPE, "position %d outside the cache (max_seq=%d)", pos, max_seq);
    if (n_splits < 1 || n_splits > 1024) return fail(AMQ_EINVAL, "n_splits must be 1..1024 (got %d)", n_splits);
    const size_t need = amq_attn_decode_kv8_workspace_bytes(batch, n_heads, n_splits);
    if (workspace_bytes < need) return fail(AMQ_EINVAL, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    // a step state carries the position and its cos/sin row: pos_dev, rope_theta and rope_table are then not looked at
    amq::Kv8Args a{q, k, v, kc8, ks, vc8, vs, out, step_state ? nullptr : pos_dev, pos, n_heads, n_kv_heads, max_seq,
                   step_state ? 10000.0f : rope_theta, step_state ? nullptr : rope_table, step_state};
    return check_hip(amq::launch_attn_decode_kv8(a, batch, n_splits, workspace, tickets, (hipStream_t)stream), "attn_decode_kv8");
}

static int amq_attn_prefill_check(const void* q, const void* k, const void* v, const void* out, int batch, int S, int pos0, int n_heads,
                                  int n_kv_heads, int head_dim, long long q_rstride, long long q_bstride, long long k_rstride,
                                  long long k_bstride, long long k_hstride, long long v_rstride, long long v_bstride, long long v_hstride,
                                  long long o_rstride, long long o_bstride) {
    if (!q || !k || !v || !out) return fail(AMQ_EINVAL, "null pointer");
    if (head_dim != 128) return fail(AMQ_ESHAPE, "head_dim must be 128 (got %d)", head_dim);
    if (batch < 1 || batch > 65535 || S < 1 || pos0 < 0 || n_heads < 1 || n_heads > 65535 || n_kv_heads < 1 || (n_heads % n_kv_heads) != 0)
        return fail(AMQ_ESHAPE, "bad sizes (batch %d, S %d, pos0 %d, %d q heads, %d kv heads)", batch, S, pos0, n_heads, n_kv_heads);
    const long long strides[] = {q_rstride, q_bstride, k_rstride, k_bstride, k_hstride, v_rstride, v_bstride, v_hstride, o_rstride, o_bstride};
    for (long long sv : strides)
        if (sv < 0 || (sv % 8) != 0) return fail(AMQ_ESHAPE, "strides must be non-negative multiples of 8 halves (16-byte vector access)");
    if (q_rstride < (long long)n_heads * 128 || o_rstride < (long long)n_heads * 128 || k_rstride < 128 || v_rstride < 128)
        return fail(AMQ_ESHAPE, "row strides smaller than the rows they separate");
    // the kernel forms key * row stride in bytes as a 24 x 24 -> 32-bit product (byte offset inside one sequence's k / v)
    const long long keys = (long long)pos0 + S;
    if (2 * k_rstride >= (1 << 24) || 2 * v_rstride >= (1 << 24) || keys >= (1 << 24) || 2 * keys * k_rstride >= (1ll << 32) || 2 * keys * v_rstride >= (1ll << 32))
        return fail(AMQ_ESHAPE, "k / v of one sequence must span fewer than 2^32 bytes (keys %lld, row strides %lld / %lld halves)", keys, k_rstride, v_rstride);
    return AMQ_OK;
}

int amq_attn_prefill_f16(const void* q, const void* k, const void* v, void* out, int batch, int S, int pos0, int n_heads,
                         int n_kv_heads, int head_dim, long long q_rstride, long long q_bstride, long long k_rstride,
                         long long k_bstride, long long k_hstride, long long v_rstride, long long v_bstride, long long v_hstride,
                         long long o_rstride, long long o_bstride, void* stream) {
    if (int rc = amq_attn_prefill_check(q, k, v, out, batch, S, pos0, n_heads, n_kv_heads, head_dim, q_rstride, q_bstride, k_rstride, k_bstride,
                                        k_hstride, v_rstride, v_bstride, v_hstride, o_rstride, o_bstride)) return rc;
    amq::AttnPrefillArgs a{q, k, v, out, S, pos0, n_heads, n_kv_heads, batch, (long)q_rstride, (long)q_bstride, (long)k_rstride,
                           (long)k_bstride, (long)k_hstride, (long)v_rstride, (long)v_bstride, (long)v_hstride, (long)o_rstride,
                           (long)o_bstride, 0};
    return check_hip(amq::launch_attn_prefill(a, (hipStream_t)stream), "attn_prefill");
}

int amq_attn_prefill_xfrag_f16(const void* q, const void* k, const void* v, void* out_xf, int S, int pos0, int n_heads,
                               int n_kv_heads, int head_dim, long long q_rstride, long long k_rstride, long long k_hstride,
                               long long v_rstride, long long v_hstride, void* stream) {
    if (int rc = amq_attn_prefill_check(q, k, v, out_xf, 1, S, pos0, n_heads, n_kv_heads, head_dim, q_rstride, 0, k_rstride, 0, k_hstride,
                                        v_rstride, 0, v_hstride, (long long)n_heads * 128, 0)) return rc;
    amq::AttnPrefillArgs a{q, k, v, out_xf, S, pos0, n_heads, n_kv_heads, 1, (long)q_rstride, 0, (long)k_rstride, 0, (long)k_hstride,
                           (long)v_rstride, 0, (long)v_hstride, 0, 0, 1};
    return check_hip(amq::launch_attn_prefill(a, (hipStream_t)stream), "attn_prefill_xfrag");
}

/* ---- token tails and set_token: ten entry points, one set of shared checks.  What differs between them is the TailForm ("Decode-step
   entry points: what is checked") and what each adds behind tail_check ---- */
enum Vocab8 { V8_NEVER, V8_TWO_ROWS, V8_ALWAYS };       // when vocab % 8 == 0 is demanded (16-byte aligned rows of logits): never / from two rows / always
struct TailForm {
    int batch_min, batch_max;
    bool blocks;            // position and cos/sin row live in an array of step-state blocks and rope_table is required;
                            // else `pos`, and rope_table / rope_cur both or neither
    Vocab8 vocab8;
    int size_code;          // the answer to vocab < 1 and batch < batch_min
    const char* rows;       // what `batch` counts, in messages
};
constexpr TailForm TAIL_ONE{1, 1, false, V8_TWO_ROWS, AMQ_ESHAPE, "batch"};
constexpr TailForm TAIL_BATCH{1, 65535, false, V8_TWO_ROWS, AMQ_ESHAPE, "batch"};
constexpr TailForm TAIL_SAMPLE{1, 8, false, V8_NEVER, AMQ_EINVAL, "rows"};          // (8: the state block holds 8 finished flags)
constexpr TailForm SET_TOKEN{1, 65535, false, V8_NEVER, AMQ_ESHAPE, "batch"};
constexpr TailForm TAIL_SEQ{1, 65535, true, V8_TWO_ROWS, AMQ_ESHAPE, "batch"};
constexpr TailForm TAIL_SAMPLE_SEQ{1, 8, true, V8_NEVER, AMQ_ESHAPE, "rows"};
constexpr TailForm SET_TOKEN_SEQ{1, 65535, true, V8_NEVER, AMQ_ESHAPE, "batch"};
constexpr TailForm TAIL_LOOKUP{2, AMQ_LOOKUP_MAX_ROWS, true, V8_ALWAYS, AMQ_ESHAPE, "rows"};

// in: logits, or set_token's token_in; state: `pos`, or the step-state blocks (then also passed as rope_cur)
static int tail_check(const TailForm& f, const void* in, int vocab, const void* embed, int hidden, const void* token, const void* state, const void* x,
                      const void* rope_table, const void* rope_cur, int rope_rows, int batch) {
    if (!in || !embed || !token || !state || !x || (f.blocks && !rope_table)) return fail(AMQ_EINVAL, "null pointer");
    if ((rope_table == nullptr) != (rope_cur == nullptr)) return fail(AMQ_EINVAL, "rope_table and rope_cur go together");
    if (rope_cur && rope_rows < 1) return fail(AMQ_EINVAL, "rope_rows must be the number of rows of rope_table");
    if (vocab < 1) return fail(f.size_code, "vocab must be >= 1 (got %d)", vocab);
    if (hidden < 8 || (hidden % 8) != 0) return fail(AMQ_ESHAPE, "need hidden >= 8 and hidden %% 8 == 0 (got %d)", hidden);
    if (batch < f.batch_min) return fail(f.size_code, "%s must be %d..%d (got %d)", f.rows, f.batch_min, f.batch_max, batch);
    if (batch > f.batch_max) return fail(AMQ_ESHAPE, "%s must be %d..%d (got %d)", f.rows, f.batch_min, f.batch_max, batch);
    if ((vocab % 8) != 0 && (f.vocab8 == V8_ALWAYS || (f.vocab8 == V8_TWO_ROWS && batch > 1)))
        return fail(AMQ_ESHAPE, "several rows need vocab %% 8 == 0 (16-byte aligned logits rows)");
    return AMQ_OK;
}
// the int32 position behind `state`: of block 0 (byte 256), or `pos` itself
static void* tail_pos(const TailForm& f, void* state) { return f.blocks ? (char*)state + 256 : state; }

// the arg-max tails (suppress_ids may be null here; rope_cur: the blocks again in the per-sequence form)
static int decode_tail(const TailForm& f, const char* what, const void* logits, int vocab, const void* embed, int hidden, long long* token, void* state,
                       void* x, const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids, void* stream) {
    if (int rc = tail_check(f, logits, vocab, embed, hidden, token, state, x, rope_table, rope_cur, rope_rows, batch)) return rc;
    return check_hip(amq::launch_decode_tail(logits, vocab, embed, hidden, token, tail_pos(f, state), x, rope_table, rope_cur, rope_rows,
                                             (hipStream_t)stream, batch, suppress_ids, f.blocks), what);
}

int amq_decode_tail_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                        const void* rope_table, void* rope_cur, int rope_rows, void* stream) {
    return decode_tail(TAIL_ONE, "decode_tail", logits, vocab, embed, hidden, token, pos, x, rope_table, rope_cur, rope_rows, 1, nullptr, stream);
}

int amq_decode_tail_batch_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                              const void* rope_table, void* rope_cur, int rope_rows, int batch, void* stream) {
    return decode_tail(TAIL_BATCH, "decode_tail_batch", logits, vocab, embed, hidden, token, pos, x, rope_table, rope_cur, rope_rows, batch, nullptr, stream);
}

int amq_decode_tail_suppress_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                                 const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids, void* stream) {
    if (!suppress_ids) return fail(AMQ_EINVAL, "suppress_ids: a device array of 8 int32 token ids (-1 = unused slot) is required");
    return decode_tail(TAIL_BATCH, "decode_tail_suppress", logits, vocab, embed, hidden, token, pos, x, rope_table, rope_cur, rope_rows, batch, suppress_ids, stream);
}

int amq_sample_f16(const void* logits, int rows, int vocab, void* state, const int* suppress_ids, const float* u_in, long long* token_out,
                   unsigned char* kept_out, int seq0, int flags, void* stream) {
    if (!state) return fail(AMQ_EINVAL, "state: the 128-byte device block of sampling parameters is required (null)");
    if (!logits || !token_out) return fail(AMQ_EINVAL, "null pointer");
    if (vocab < 1) return fail(AMQ_EINVAL, "vocab must be >= 1 (got %d)", vocab);
    if (rows < 1) return fail(AMQ_EINVAL, "rows must be >= 1 (got %d)", rows);
    if (flags & ~3) return fail(AMQ_EINVAL, "unknown flags %d", flags);
    if ((flags & AMQ_SAMPLE_EOS) && rows > 8) return fail(AMQ_ESHAPE, "EOS bookkeeping serves at most 8 sequences (the state block holds 8 flags), got %d rows", rows);
    if ((long long)rows * vocab >= (1ll << 40)) return fail(AMQ_ESHAPE, "rows * vocab too large");
    amq::SampleArgs a{(const _Float16*)logits, vocab, nullptr, 0, token_out, nullptr, nullptr, nullptr, nullptr, 0, suppress_ids, (int*)state,
                      u_in, kept_out, seq0, flags};
    return check_hip(amq::launch_sample(a, rows, (hipStream_t)stream), "sample");
}

/* ---- evaluation metrics over rows of logits (amq_eval.hip) ---- */
static int check_logit_rows(int M, int V, long long stride, const char* which) {
    if (M < 1) return fail(AMQ_EINVAL, "M (rows) must be >= 1 (got %d)", M);
    if (V < 1) return fail(AMQ_EINVAL, "V (vocabulary) must be >= 1 (got %d)", V);
    if (stride < (long long)V) return fail(AMQ_ESHAPE, "%s: a row stride of %lld elements is shorter than a row of V = %d", which, stride, V);
    return AMQ_OK;
}

int amq_logit_nll_f16(const void* logits, long long row_stride, const long long* labels, int M, int V, float* nll_out, float* lse_out,
                      int* argmax_out, void* stream) {
    if (!logits || !nll_out) return fail(AMQ_EINVAL, "null pointer (logits and nll_out are required)");
    if (int rc = check_logit_rows(M, V, row_stride, "row_stride")) return rc;
    return check_hip(amq::launch_logit_nll(logits, row_stride, labels, M, V, nll_out, lse_out, argmax_out, (hipStream_t)stream), "logit_nll");
}

int amq_logit_jsd_f16(const void* p, long long p_stride, const void* q, long long q_stride, int q_is_f32, int M, int V, float eps, float* jsd_out,
                      void* stream) {
    if (!p || !q || !jsd_out) return fail(AMQ_EINVAL, "null pointer");
    if (q_is_f32 != 0 && q_is_f32 != 1) return fail(AMQ_EINVAL, "q_is_f32 must be 0 (fp16 q) or 1 (fp32 q), got %d", q_is_f32);
    if (!(eps >= 0.0f)) return fail(AMQ_EINVAL, "eps must be >= 0");
    if (int rc = check_logit_rows(M, V, p_stride, "p_stride")) return rc;
    if (int rc = check_logit_rows(M, V, q_stride, "q_stride")) return rc;
    return check_hip(amq::launch_logit_jsd(p, p_stride, q, q_stride, q_is_f32 != 0, M, V, eps, jsd_out, (hipStream_t)stream), "logit_jsd");
}

// the sampled tails
static int decode_tail_sample(const TailForm& f, const char* what, const void* logits, int vocab, const void* embed, int hidden, long long* token,
                              void* state, void* x, const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids,
                              void* sampling, void* stream) {
    if (!sampling) return fail(AMQ_EINVAL, "state: the 128-byte device block of sampling parameters is required (null)");
    if (int rc = tail_check(f, logits, vocab, embed, hidden, token, state, x, rope_table, rope_cur, rope_rows, batch)) return rc;
    amq::SampleArgs a{(const _Float16*)logits, vocab, (const _Float16*)embed, hidden, token, (int*)tail_pos(f, state), (_Float16*)x,
                      (const _Float16*)rope_table, (_Float16*)rope_cur, rope_rows, suppress_ids, (int*)sampling, nullptr, nullptr, 0,
                      AMQ_SAMPLE_ADVANCE | AMQ_SAMPLE_EOS};
    return check_hip(amq::launch_sample(a, batch, (hipStream_t)stream, f.blocks), what);
}

int amq_decode_tail_sample_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, int* pos, void* x,
                               const void* rope_table, void* rope_cur, int rope_rows, int batch, const int* suppress_ids, void* state,
                               void* stream) {
    return decode_tail_sample(TAIL_SAMPLE, "decode_tail_sample", logits, vocab, embed, hidden, token, pos, x, rope_table, rope_cur, rope_rows, batch, suppress_ids, state, stream);
}

static int set_token(const TailForm& f, const char* what, const long long* token_in, int n_in, const void* embed, int vocab, int hidden, long long* token,
                     void* state, void* x, const void* rope_table, void* rope_cur, int rope_rows, int batch, void* stream) {
    if (int rc = tail_check(f, token_in, vocab, embed, hidden, token, state, x, rope_table, rope_cur, rope_rows, batch)) return rc;
    if (n_in != 1 && n_in != batch) return fail(AMQ_ESHAPE, "batch %d with %d input ids (1 or one per sequence)", batch, n_in);
    return check_hip(amq::launch_set_token(token_in, n_in, embed, vocab, hidden, token, tail_pos(f, state), x, rope_table, rope_cur, rope_rows, batch,
                                           (hipStream_t)stream, f.blocks), what);
}

int amq_set_token_f16(const long long* token_in, int n_in, const void* embed, int vocab, int hidden, long long* token, const int* pos, void* x,
                      const void* rope_table, void* rope_cur, int rope_rows, int batch, void* stream) {
    return set_token(SET_TOKEN, "set_token", token_in, n_in, embed, vocab, hidden, token, (void*)pos, x, rope_table, rope_cur, rope_rows, batch, stream);
}

/* ---- sequences at positions of their own: an array of `batch` step-state blocks AMQ_STEP_STATE_STRIDE bytes apart ---- */
static_assert(AMQ_STEP_STATE_STRIDE == amq::STEP_STRIDE && AMQ_STEP_STATE_STRIDE % 16 == 0 && AMQ_STEP_STATE_STRIDE >= 264, "step-state stride");

int amq_attn_decode_seq_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int batch,
                            int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                            void* tickets, void* stream) {
    return amq_attn_decode_seq_qkn_f16(nullptr, q, k, v, kcache, vcache, out, step_states, batch, n_heads, n_kv_heads, head_dim, max_seq, n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_attn_decode_seq_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                void* step_states, int batch, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    return attn_decode(ATTN_SEQ, norm, q, k, v, kcache, vcache, out, step_states, nullptr, 0, batch, n_heads, n_kv_heads, head_dim, max_seq, 10000.0f, nullptr,
                       n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_decode_tail_seq_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                            const void* rope_table, int rope_rows, int batch, const int* suppress_ids, void* stream) {
    return decode_tail(TAIL_SEQ, "decode_tail_seq", logits, vocab, embed, hidden, token, step_states, x, rope_table, step_states, rope_rows, batch, suppress_ids, stream);
}

int amq_decode_tail_sample_seq_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                                   const void* rope_table, int rope_rows, int batch, const int* suppress_ids, void* state, void* stream) {
    return decode_tail_sample(TAIL_SAMPLE_SEQ, "decode_tail_sample_seq", logits, vocab, embed, hidden, token, step_states, x, rope_table, step_states, rope_rows, batch,
                              suppress_ids, state, stream);
}

int amq_set_token_seq_f16(const long long* token_in, int n_in, const void* embed, int vocab, int hidden, long long* token, void* step_states, void* x,
                          const void* rope_table, int rope_rows, int batch, void* stream) {
    return set_token(SET_TOKEN_SEQ, "set_token_seq", token_in, n_in, embed, vocab, hidden, token, step_states, x, rope_table, step_states, rope_rows, batch, stream);
}

/* ---- prompt-lookup speculative decoding: `rows` consecutive positions of ONE sequence per step ---- */
static_assert(AMQ_LOOKUP_STATE_WORDS == amq::LK_WORDS && AMQ_LOOKUP_MAX_ROWS == 8, "lookup state block");

int amq_attn_decode_rows_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int rows,
                             int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                             void* tickets, void* stream) {
    return amq_attn_decode_rows_qkn_f16(nullptr, q, k, v, kcache, vcache, out, step_states, rows, n_heads, n_kv_heads, head_dim, max_seq, n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_attn_decode_rows_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                 void* step_states, int rows, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                 void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    return attn_decode(ATTN_ROWS, norm, q, k, v, kcache, vcache, out, step_states, nullptr, 0, rows, n_heads, n_kv_heads, head_dim, max_seq, 10000.0f, nullptr,
                       n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_attn_decode_rows_gqa_f16(const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out, void* step_states, int rows,
                                 int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits, void* workspace, size_t workspace_bytes,
                                 void* tickets, void* stream) {
    return amq_attn_decode_rows_gqa_qkn_f16(nullptr, q, k, v, kcache, vcache, out, step_states, rows, n_heads, n_kv_heads, head_dim, max_seq, n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_attn_decode_rows_gqa_qkn_f16(const amq_qk_norm* norm, const void* q, const void* k, const void* v, void* kcache, void* vcache, void* out,
                                     void* step_states, int rows, int n_heads, int n_kv_heads, int head_dim, int max_seq, int n_splits,
                                     void* workspace, size_t workspace_bytes, void* tickets, void* stream) {
    return attn_decode(ATTN_ROWS_GQA, norm, q, k, v, kcache, vcache, out, step_states, nullptr, 0, rows, n_heads, n_kv_heads, head_dim, max_seq, 10000.0f, nullptr,
                       n_splits, workspace, workspace_bytes, tickets, stream);
}

int amq_decode_tail_lookup_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                               const void* rope_table, int rope_rows, int rows, const int* suppress_ids, void* lookup_state, int* history,
                               int history_cap, void* stream) {
    if (!lookup_state || !history) return fail(AMQ_EINVAL, "lookup_state (the 128-byte device block) and history are required (null)");
    if (int rc = tail_check(TAIL_LOOKUP, logits, vocab, embed, hidden, token, step_states, x, rope_table, step_states, rope_rows, rows)) return rc;
    if (history_cap < rope_rows || history_cap > (1 << 24))
        return fail(AMQ_ESHAPE, "history_cap must hold the whole cache (max_seq = rope_rows = %d) and at most 2^24 tokens, got %d", rope_rows, history_cap);
    amq::LookupArgs a{(const _Float16*)logits, vocab, (const _Float16*)embed, hidden, token, step_states, (_Float16*)x, (const _Float16*)rope_table,
                      rope_rows, suppress_ids, (int*)lookup_state, history, history_cap};
    return check_hip(amq::launch_decode_tail_lookup(a, rows, (hipStream_t)stream), "decode_tail_lookup");
}

int amq_decode_tail_lookup_sample_f16(const void* logits, int vocab, const void* embed, int hidden, long long* token, void* step_states, void* x,
                                      const void* rope_table, int rope_rows, int rows, const int* suppress_ids, void* lookup_state, int* history,
                                      int history_cap, void* sample_state, const float* u_in, unsigned char* kept_out, void* stream) {
    if (!sample_state) return fail(AMQ_EINVAL, "sample_state: the 128-byte device block of sampling parameters is required (null)");
    if (!lookup_state || !history) return fail(AMQ_EINVAL, "lookup_state (the 128-byte device block) and history are required (null)");
    if (int rc = tail_check(TAIL_LOOKUP, logits, vocab, embed, hidden, token, step_states, x, rope_table, step_states, rope_rows, rows)) return rc;
    if (history_cap < rope_rows || history_cap > (1 << 24))
        return fail(AMQ_ESHAPE, "history_cap must hold the whole cache (max_seq = rope_rows = %d) and at most 2^24 tokens, got %d", rope_rows, history_cap);
    amq::LookupSampleArgs a{{(const _Float16*)logits, vocab, (const _Float16*)embed, hidden, token, step_states, (_Float16*)x,
                             (const _Float16*)rope_table, rope_rows, suppress_ids, (int*)lookup_state, history, history_cap},
                            (int*)sample_state, u_in, kept_out};
    return check_hip(amq::launch_decode_tail_lookup_sample(a, rows, (hipStream_t)stream), "decode_tail_lookup_sample");
}

int amq_rope_table_f16(void* table, int max_seq, float rope_theta, void* stream) {
    if (!table || max_seq < 1) return fail(AMQ_EINVAL, "bad rope table request");
    return check_hip(amq::launch_rope_table(table, max_seq, rope_theta, (hipStream_t)stream), "rope_table");
}

int amq_rope_table_freqs_f16(void* table, int max_seq, const float* inv_freq, float scale, void* stream) {
    if (!table || !inv_freq || max_seq < 1) return fail(AMQ_EINVAL, "bad rope table request");
    return check_hip(amq::launch_rope_table_freqs(table, max_seq, inv_freq, scale, (hipStream_t)stream), "rope_table_freqs");
}

}  // extern "C"
