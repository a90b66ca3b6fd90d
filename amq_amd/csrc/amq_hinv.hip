// amq_hinv.hip -- the upper Cholesky factor U of the damped inverse Hessian (U^T U = A^-1) as HIP kernels, DESIGN.md 3.10.1.
//
// A = R R^T with R UPPER triangular (a Cholesky factorisation that starts at the bottom-right corner and walks up-left); then A^-1 = R^-T R^-1 and,
// the upper factor being unique, U = R^-1: one factorisation (K^3 / 3) and one triangular inverse (K^3 / 3), no explicit A^-1, fp32 throughout.
//
// Everything works on matrices PADDED at the top-left to Kp = ceil(K / 64) * 64 rows: padded index p = i + (Kp - K), the padding carries the
// identity, diag(I, A) = diag(I, R) diag(I, R)^T and diag(I, R)^-1 = diag(I, U).  So every tile of every kernel is a full 64 x 64 tile, the partial
// block of a K that is no multiple of 64 sits at the top-left where the backward walk ends, and only hinv_copy_in / hinv_copy_out know K.
//
//   hinv_prepare   one workgroup: zeroes the info block, writes the dead mask (walk order), sums the diagonal (dead entries as 1) in a fixed order
//                  in fp64 and leaves damp = percdamp * mean, rounded once to fp32, in the workspace.
//   hinv_copy_in   one workgroup per upper tile: A[p][q] = H[perm[i]][perm[j]] of H's upper triangle in walk order (the lower halves of the diagonal
//                  tiles mirror it), dead diagonal -> 1, + damp; a non-finite entry raises info[0].
//   hinv_panel     step b = nb - 1 .. 0, max(b, 1) workgroups: EVERY workgroup factors the diagonal block A_bb = R_bb R_bb^T in LDS (column by column
//                  from the last, correctly rounded sqrt and division), inverts R_bb there to T_b (row by row from the last), and forms its row tile
//                  of the panel as a product R_ib = A_ib T_b^T on v_mfma_f32_32x32x2_f32.  The redundant factorisations are bit-identical and save a
//                  launch and a grid-wide dependency per step.  Workgroup 0 stores T_b = U_bb as the diagonal tile of the second matrix and reports
//                  a failed pivot (<= 0 or not finite; the kernel carries on with 1).
//   hinv_trailing  A_ij -= R_ib R_jb^T for the tiles i <= j < b, one workgroup per tile, operands staged through LDS, accumulators in registers.
//   hinv_finish    column j of the inverse, j workgroups: U_ij = -S_ij T_j.
//   hinv_spread    (j + 1) x (nb - 1 - j) workgroups: S_ij' (+)= U_ij R_jj' for i <= j < j' -- the right-looking form of
//                  U_{0:j, j} = -U_{0:j, 0:j} R_{0:j, j} T_j: every launch is one k-step of every tile it touches, as wide as the trailing update.
//   hinv_copy_out  U [K, K] from the second matrix, the strict lower triangle as exact zeros.
//
// No atomics; the grids and every summation order depend on K alone, so a run gives the same bits as the next.  Waits are the compiler's.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int NB = HINV_NB;          // block = tile = 64
constexpr int PITCH = NB + 2;        // LDS row pitch in floats: rows stay 8-byte aligned, and 66 l mod 64 = 2 l spreads the 32 rows a wave reads
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct alignas(16) Tile { float v[NB][PITCH]; };

// global tile (row-major, leading dimension ld) -> LDS, as it is or transposed; 256 threads, 16-byte loads
template <bool TRANSPOSE>
__device__ __forceinline__ void stage(Tile& s, const float* __restrict__ g, size_t ld) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = (int)threadIdx.x + 256 * e;       // 1024 float4 pieces
        const int r = idx >> 4, c = (idx & 15) * 4;
        const float4 x = *(const float4*)(g + (size_t)r * ld + c);
        if (TRANSPOSE) {
            s.v[c][r] = x.x; s.v[c + 1][r] = x.y; s.v[c + 2][r] = x.z; s.v[c + 3][r] = x.w;
        } else {
            *(float2*)&s.v[r][c] = make_float2(x.x, x.y);
            *(float2*)&s.v[r][c + 2] = make_float2(x.z, x.w);
        }
    }
}

// acc (the wave's 32 x 32 quadrant of the 64 x 64 tile) += X Y^T: X = sx[m][k], Y = sy[n][k].  One 8-byte read per operand feeds two MFMAs: half
// h = lane / 32 of the wave holds k = 4 s + 2 h, 4 s + 2 h + 1, the same on both sides, so each instruction sums two matching k.
__device__ __forceinline__ void mma_tile(f32x16& acc, const Tile& sx, const Tile& sy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* px = &sx.v[(wave >> 1) * 32 + (lane & 31)][2 * (lane >> 5)];
    const float* py = &sy.v[(wave & 1) * 32 + (lane & 31)][2 * (lane >> 5)];
#pragma unroll
    for (int s = 0; s < NB / 4; ++s) {
        const float2 a = *(const float2*)(px + 4 * s), b = *(const float2*)(py + 4 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    }
}

// element v of the wave's accumulator is row acc_row(v), column acc_col() of the tile
__device__ __forceinline__ int acc_row(int v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return (wave >> 1) * 32 + (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3);
}
__device__ __forceinline__ int acc_col() { return ((threadIdx.x >> 6) & 1) * 32 + (threadIdx.x & 31); }

enum { OUT_SET, OUT_NEG, OUT_ADD, OUT_SUB };
template <int MODE>
__device__ __forceinline__ void store_acc(float* __restrict__ g, size_t ld, const f32x16& acc) {
    const int n = acc_col();
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        float* p = g + (size_t)acc_row(v) * ld + n;
        if (MODE == OUT_SET) *p = acc[v];
        if (MODE == OUT_NEG) *p = -acc[v];
        if (MODE == OUT_ADD) *p = *p + acc[v];
        if (MODE == OUT_SUB) *p = *p - acc[v];
    }
}

__device__ __forceinline__ const float* tile_of(const float* M, size_t Kp, int i, int j) { return M + ((size_t)i * Kp + j) * NB; }
__device__ __forceinline__ float* tile_of(float* M, size_t Kp, int i, int j) { return M + ((size_t)i * Kp + j) * NB; }

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }      // false for inf and NaN

// entry i of perm, or i; an entry outside 0 .. K - 1 is read as 0 and raises info[0] (the caller guarantees a permutation)
__device__ __forceinline__ int walk(const int* __restrict__ perm, int i, int K, int* __restrict__ info) {
    if (!perm) return i;
    int p = perm[i];
    if ((unsigned)p >= (unsigned)K) { p = 0; info[0] = 1; }
    return p;
}

__global__ __launch_bounds__(256) void hinv_prepare_kernel(const float* __restrict__ H, const int* __restrict__ perm, int K, float percdamp,
                                                           uint8_t* __restrict__ dead, int* __restrict__ info, float* __restrict__ damp) {
    __shared__ double part[256];
    if (threadIdx.x < HINV_INFO_BYTES / 4) info[threadIdx.x] = 0;
    __syncthreads();                                      // (walk() may raise info[0] below)
    // thread t sums the entries t, t + 256, ... ascending; the 256 partial sums are added pairwise in a fixed tree
    double sum = 0.0;
    for (int i = threadIdx.x; i < K; i += 256) {
        const int p = walk(perm, i, K, info);
        const float d = H[(size_t)p * K + p];
        dead[i] = d == 0.0f;
        sum += d == 0.0f ? 1.0 : (double)d;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) damp[0] = (float)((double)percdamp * (part[0] / (double)K));
}

__global__ __launch_bounds__(256) void hinv_copy_in_kernel(const float* __restrict__ H, const int* __restrict__ perm, int K, int Kp,
                                                           const float* __restrict__ damp, float* __restrict__ A, int* __restrict__ info) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                   // only the upper tiles exist
    const int shift = Kp - K;
    const float dmp = damp[0];
    bool bad = false;
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int p = ti * NB + (e >> 6), q = tj * NB + (e & 63);
        float x;
        if (p < shift || q < shift) {
            x = p == q ? 1.0f : 0.0f;
        } else {
            const int i = min(p, q) - shift, j = max(p, q) - shift;      // H's upper triangle in walk order
            x = H[(size_t)walk(perm, i, K, info) * K + walk(perm, j, K, info)];
            bad |= !finite_f(x);
            if (i == j) x = (x == 0.0f ? 1.0f : x) + dmp;
        }
        A[(size_t)p * Kp + q] = x;
    }
    if (bad) info[0] = 1;
}

__global__ __launch_bounds__(256) void hinv_panel_kernel(float* __restrict__ A, float* __restrict__ Um, int Kp, int K, int b, int* __restrict__ info) {
    __shared__ Tile sA, sT, sX;
    __shared__ float piv[NB];
    const int tid = threadIdx.x, i = blockIdx.x;
    stage<false>(sA, tile_of(A, Kp, b, b), Kp);
    if (i < b) stage<false>(sX, tile_of(A, Kp, i, b), Kp);
    for (int e = tid; e < NB * NB; e += 256) sT.v[e >> 6][e & 63] = 0.0f;

    // A_bb = R_bb R_bb^T, column by column from the last: R[c][c] = sqrt(A[c][c]), R[r][c] = A[r][c] / R[c][c], A[r][s] -= R[r][c] R[s][c] (r <= s < c)
    for (int c = NB - 1; c >= 0; --c) {
        __syncthreads();
        const float d = sA.v[c][c];
        const bool fail = !(d > 0.0f) || !finite_f(d);
        const float rcc = fail ? 1.0f : sqrtf(d);
        if (tid < c) sA.v[tid][c] = sA.v[tid][c] / rcc;
        if (tid == c) {
            piv[c] = rcc;
            if (fail && i == 0 && info[1] == 0) { info[1] = 1; info[2] = b * NB + c - (Kp - K); }
        }
        __syncthreads();
        const int s = tid & 63;
        if (s < c) {
            const float rs = sA.v[s][c];
            for (int r = tid >> 6; r <= s; r += 4) sA.v[r][s] = fmaf(-sA.v[r][c], rs, sA.v[r][s]);
        }
    }
    __syncthreads();
    if (tid < NB) { sA.v[tid][tid] = piv[tid]; sT.v[tid][tid] = 1.0f / piv[tid]; }

    // T = R_bb^-1, row by row from the last: T[r][c] = -(sum_{k = r + 1 .. c} R[r][k] T[k][c]) / R[r][r].  Four neighbouring lanes share a column:
    // lane part q sums k = r + 1 + q, + 4, ... ascending, then (q0 + q1) + (q2 + q3)
    {
        const int c = tid >> 2, q = tid & 3;
        for (int r = NB - 2; r >= 0; --r) {
            __syncthreads();
            float sum = 0.0f;
            for (int k = r + 1 + q; k <= c; k += 4) sum = fmaf(sA.v[r][k], sT.v[k][c], sum);
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            if (q == 0 && c > r) sT.v[r][c] = -sum / sA.v[r][r];
        }
    }
    __syncthreads();

    if (i == 0) {                                          // U_bb = T_b
        float* u = tile_of(Um, Kp, b, b);
        for (int e = tid; e < NB * NB; e += 256) u[(size_t)(e >> 6) * Kp + (e & 63)] = sT.v[e >> 6][e & 63];
    }
    if (i < b) {                                           // R_ib = A_ib T_b^T
        f32x16 acc = {};
        mma_tile(acc, sX, sT);
        store_acc<OUT_SET>(tile_of(A, Kp, i, b), Kp, acc);
    }
}

__global__ __launch_bounds__(256) void hinv_trailing_kernel(float* __restrict__ A, int Kp, int b) {
    __shared__ Tile sX, sY;
    // linear index t -> the tile (i, j), i <= j: t = j (j + 1) / 2 + i
    const int t = blockIdx.x;
    int j = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (j * (j + 1) / 2 > t) --j;
    while ((j + 1) * (j + 2) / 2 <= t) ++j;
    const int i = t - j * (j + 1) / 2;
    stage<false>(sX, tile_of(A, Kp, i, b), Kp);
    stage<false>(sY, tile_of(A, Kp, j, b), Kp);
    __syncthreads();
    f32x16 acc = {};
    mma_tile(acc, sX, sY);
    store_acc<OUT_SUB>(tile_of(A, Kp, i, j), Kp, acc);
}

__global__ __launch_bounds__(256) void hinv_finish_kernel(float* __restrict__ Um, int Kp, int j) {
    __shared__ Tile sX, sY;
    const int i = blockIdx.x;
    stage<false>(sX, tile_of(Um, Kp, i, j), Kp);            // S_ij [m][k]
    stage<true>(sY, tile_of(Um, Kp, j, j), Kp);             // T_j [k][n] -> [n][k]
    __syncthreads();
    f32x16 acc = {};
    mma_tile(acc, sX, sY);
    store_acc<OUT_NEG>(tile_of(Um, Kp, i, j), Kp, acc);
}

__global__ __launch_bounds__(256) void hinv_spread_kernel(const float* __restrict__ A, float* __restrict__ Um, int Kp, int j) {
    __shared__ Tile sX, sY;
    const int i = blockIdx.y, jj = j + 1 + blockIdx.x;
    stage<false>(sX, tile_of(Um, Kp, i, j), Kp);            // U_ij [m][k]
    stage<true>(sY, tile_of(A, Kp, j, jj), Kp);             // R_jj' [k][n] -> [n][k]
    __syncthreads();
    f32x16 acc = {};
    mma_tile(acc, sX, sY);
    if (i == j) store_acc<OUT_SET>(tile_of(Um, Kp, i, jj), Kp, acc);      // the tile's first term
    else store_acc<OUT_ADD>(tile_of(Um, Kp, i, jj), Kp, acc);
}

__global__ __launch_bounds__(256) void hinv_copy_out_kernel(const float* __restrict__ Um, int K, int Kp, float* __restrict__ U) {
    const int shift = Kp - K;
    const int i = blockIdx.y;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < K; j += gridDim.x * 256)
        U[(size_t)i * K + j] = j >= i ? Um[(size_t)(i + shift) * Kp + (j + shift)] : 0.0f;
}

}  // namespace

hipError_t launch_gptq_hinv(const void* H, const void* perm, int K, float percdamp, void* U, void* dead, void* info, void* workspace,
                            hipStream_t st) {
    const int nb = hinv_blocks(K), Kp = nb * NB;
    float* A = (float*)workspace;
    float* Um = A + (size_t)Kp * Kp;
    float* damp = Um + (size_t)Kp * Kp;
    int* inf = (int*)info;
    hipLaunchKernelGGL(hinv_prepare_kernel, dim3(1), dim3(256), 0, st, (const float*)H, (const int*)perm, K, percdamp, (uint8_t*)dead, inf, damp);
    hipLaunchKernelGGL(hinv_copy_in_kernel, dim3(nb, nb), dim3(256), 0, st, (const float*)H, (const int*)perm, K, Kp, damp, A, inf);
    for (int b = nb - 1; b >= 0; --b) {
        hipLaunchKernelGGL(hinv_panel_kernel, dim3(b > 0 ? b : 1), dim3(256), 0, st, A, Um, Kp, K, b, inf);
        if (b > 0) hipLaunchKernelGGL(hinv_trailing_kernel, dim3(b * (b + 1) / 2), dim3(256), 0, st, A, Kp, b);
    }
    for (int j = 0; j < nb; ++j) {
        if (j > 0) hipLaunchKernelGGL(hinv_finish_kernel, dim3(j), dim3(256), 0, st, Um, Kp, j);
        if (j < nb - 1) hipLaunchKernelGGL(hinv_spread_kernel, dim3(nb - 1 - j, j + 1), dim3(256), 0, st, A, Um, Kp, j);
    }
    hipLaunchKernelGGL(hinv_copy_out_kernel, dim3((K + 1023) / 1024, K), dim3(256), 0, st, Um, K, Kp, (float*)U);
    return hipGetLastError();
}

}  // namespace amq
