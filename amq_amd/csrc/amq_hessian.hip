// amq_hessian.hip -- the running Hessian of a linear's inputs, H <- H n / (n + b) + (2 / (n + b)) X^T X, as one kernel on the fp16 matrix
// instructions.  X fp16 [T, K] (the b sequences of one call, flattened), H fp32 [K, K].
//
// A symmetric rank-T update: only the 128 x 128 tiles on or above the diagonal are computed, one workgroup (four waves) per tile, the whole
// token range in one pass (no split of T: no workspace, no second rounding chain).  H's upper triangle is read once (not at all when n == 0) and
// every element of H is written once: the tile, and its mirror with the same bits.
//
//   staging   the reduction runs over tokens, the strided dimension of X.  Panels of TS = 32 tokens x 128 columns go global -> registers -> LDS
//             with 16-byte loads along K (16 neighbouring threads read 256 contiguous bytes of a token row); the loads of step s + 1 are issued
//             before the matrix instructions of step s and land in the other LDS buffer after them: two steps in flight, one barrier per step.
//             Tokens beyond T and columns beyond K are zeros in LDS.  A diagonal tile stages one panel and reads both operands from it.
//   operands  v_mfma_f32_32x32x16_f16 wants, per lane, 8 consecutive tokens of ONE column (A: m = lane & 31, k = 8 (lane >> 5) + j; B the same
//             with n) while LDS rows are tokens: two ds_read_b64_tr_b16 per operand.  In a 16-lane group lane 4 q + p gives the address of row q,
//             columns 4 p .. 4 p + 3 of a 4-token x 16-column block and receives column (lane & 15) of the four rows.  Both operands are formed
//             by the same read, so whichever order the four tokens arrive in, A's k is B's k.  Row pitch 144 halves (288 bytes): the four rows a
//             group addresses start 8 banks apart.
//   tile      each wave owns a 64 x 64 quarter as 2 x 2 accumulators of 32 x 32 (64 registers): per 16 tokens four operand fragments feed four
//             MFMAs.  On a diagonal tile the wave below the diagonal skips its products (it still stages).
//   epilogue  out = acc * fp32(2 / (n + b)) + H_old * fp32(n / (n + b)): three roundings, written out (-ffp-contract=off); the factors are
//             rounded once from double on the host.  An accumulator lane holds 4 consecutive rows of one column: the tile is stored by rows
//             (32 lanes = 128 contiguous bytes), the mirror as one 16-byte store per lane.  On a diagonal tile only row <= column is read,
//             formed and written (and mirrored): H == H^T by construction.
//
// No atomics, no workspace; the grid and every summation order depend on (T, K) alone.  Waits are the compiler's.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int TILE = HESS_TILE;      // output tile of a workgroup: 128 x 128
constexpr int TS = 32;               // tokens per staging step
constexpr int PITCH = TILE + 16;     // LDS row pitch in halves
typedef __fp16 v4h __attribute__((__vector_size__(4 * sizeof(__fp16))));      // the transposing read's own result type

struct alignas(16) Panel { _Float16 v[TS][PITCH]; };

// the two 16-byte pieces this thread moves per panel and step: piece c = tid + 256 e is token c / 16, columns 8 (c % 16) .. + 7
__device__ __forceinline__ void fetch(u4 (&r)[2], const _Float16* __restrict__ x, long stride, int T, int K, int t0, int c0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = (int)threadIdx.x + 256 * e;
        const int tok = t0 + (c >> 4), col = c0 + 8 * (c & 15);
        r[e] = (u4){0u, 0u, 0u, 0u};
        if (tok < T && col < K) r[e] = *(const u4*)(x + (size_t)tok * (size_t)stride + col);      // K % 8 == 0: a piece is inside or outside
    }
}
__device__ __forceinline__ void put(Panel& p, const u4 (&r)[2]) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = (int)threadIdx.x + 256 * e;
        *(u4*)&p.v[c >> 4][8 * (c & 15)] = r[e];
    }
}

// operand fragment of columns cb .. cb + 31, tokens tb .. tb + 15 of the panel: lane l gets column cb + (l & 31), tokens tb + 8 (l >> 5) + 0 .. 7
__device__ __forceinline__ h8 frag(const Panel& p, int tb, int cb) {
    const int lane = threadIdx.x & 63;
    const int tok = tb + 8 * (lane >> 5) + ((lane & 15) >> 2), col = cb + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const v4h lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) v4h*)&p.v[tok][col]);
    const v4h hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) v4h*)&p.v[tok + 4][col]);
    return (h8){(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
}

__global__ __launch_bounds__(256) void hessian_kernel(const _Float16* __restrict__ x, long stride, int T, int K, float* __restrict__ H,
                                                       float s_old, float s_new, int read_old) {
    __shared__ Panel sm[2][2];       // [buffer][row panel, column panel]
    // linear index t -> the tile (ti, tj), ti <= tj: t = tj (tj + 1) / 2 + ti
    const int t = blockIdx.x;
    int tj = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (tj * (tj + 1) / 2 > t) --tj;
    while ((tj + 1) * (tj + 2) / 2 <= t) ++tj;
    const int ti = t - tj * (tj + 1) / 2;
    const bool diag = ti == tj;
    const int I = ti * TILE, J = tj * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const bool works = !(diag && wr > wc);                 // the quarter below the diagonal of a diagonal tile is never stored
    const int steps = (T + TS - 1) / TS;

    f16v acc[2][2] = {};
    u4 ra[2], rb[2];
    fetch(ra, x, stride, T, K, 0, I);
    if (!diag) fetch(rb, x, stride, T, K, 0, J);
    put(sm[0][0], ra);
    if (!diag) put(sm[0][1], rb);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < steps;
        if (more) {
            fetch(ra, x, stride, T, K, (s + 1) * TS, I);
            if (!diag) fetch(rb, x, stride, T, K, (s + 1) * TS, J);
        }
        if (works) {
            const Panel& pa = sm[cur][0];
            const Panel& pb = sm[cur][diag ? 0 : 1];
#pragma unroll
            for (int ks = 0; ks < TS / 16; ++ks) {
                const h8 a0 = frag(pa, 16 * ks, 64 * wr), a1 = frag(pa, 16 * ks, 64 * wr + 32);
                const h8 b0 = frag(pb, 16 * ks, 64 * wc), b1 = frag(pb, 16 * ks, 64 * wc + 32);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (more) {                                        // the other buffer: every wave left it at the barrier that ended step s - 1
            put(sm[cur ^ 1][0], ra);
            if (!diag) put(sm[cur ^ 1][1], rb);
        }
        __syncthreads();
    }
    if (!works) return;

    // element v of acc[a][b]: row I + 64 wr + 32 a + 8 (v / 4) + 4 (lane / 32) + v % 4, column J + 64 wc + 32 b + lane % 32
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = J + 64 * wc + 32 * b + (lane & 31);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row0 = I + 64 * wr + 32 * a + 8 * g + 4 * (lane >> 5);
                if (col >= K || row0 >= K) continue;       // K % 4 == 0: the four rows are inside or outside together
                float out[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = row0 + i;
                    out[i] = acc[a][b][4 * g + i] * s_new;
                    if (diag && row > col) continue;
                    float* p = H + (size_t)row * K + col;
                    if (read_old) out[i] = out[i] + *p * s_old;
                    *p = out[i];
                }
                float* m = H + (size_t)col * K + row0;      // the mirror: H[col][row0 .. row0 + 3]
                if (!diag) {
                    *(f4*)m = (f4){out[0], out[1], out[2], out[3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (row0 + i < col) m[i] = out[i];
                }
            }
        }
}

}  // namespace

hipError_t launch_gptq_hessian(const void* x, long x_row_stride, int T, int K, void* H, int n_before, int b, hipStream_t st) {
    const int nt = (K + TILE - 1) / TILE;
    const double n = (double)n_before + (double)b;
    const float s_old = (float)((double)n_before / n), s_new = (float)(2.0 / n);
    hipLaunchKernelGGL(hessian_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, (const _Float16*)x, x_row_stride, T, K, (float*)H, s_old, s_new,
                       n_before > 0 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace amq
