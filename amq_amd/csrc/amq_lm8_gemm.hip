// amq_lm8_gemm.hip -- the 8-bit lm_head ("LM8") on the matrix cores: y [M, N] = (RMSNorm'ed) x [M, K] . W^T for 1 <= M <= 16 rows of x
// over the layer's bytes as amq_lm8.hip reads them (codes uint8 [N, K] row-major, meta fp16 [N, K / 128, 2]; no repacked copy, no workspace).
// lm8_gemv_kernel forms a dot product per row of x behind every unpacked weight; here the unpacked weights are the A operand of
// v_mfma_f32_16x16x32_f16 and the rows of x its 16 B columns: the work behind the unpack is the same for 1 row or 16.
//
//   tile      a wave owns 16 vocabulary rows and walks the whole K for them; tiles go to waves grid-stride (the 16 waves of a workgroup take 16
//             adjacent tiles: 16 x 16 x K contiguous bytes).  One 16 x 16 fp32 accumulator (4 registers), no cross-wave reduction, no atomics: the
//             same bits run to run.  A lane (r = lane % 16, g = lane / 16) ends with y[m = r][16 t + 4 g + i], i = 0 .. 3.
//   k order   both operands permute k the same way.  Per 64-k step (k0) lane (r, g) loads 16 B = the codes k0 + 16 g .. + 15 of vocabulary row
//             16 t + r: the first 8 are its k-slots 8 g .. 8 g + 7 of one MFMA, the last 8 those of the next.  Two adjacent steps = one group of
//             128 = one (scale, zero) dword per lane are issued together (the 16 rows' two 64-byte segments are one 128-byte line each); LG_D groups
//             are in flight under the arithmetic of the LG_D before them (two register buffers), non-temporal.
//   unpack    v_perm_b32 puts a byte under 0x64: the half 1024 + c, minus 1024 -- exact (integers below 2048), the value lm8_pair (amq_lm8.hip)
//             forms -- then fp16(c - zero), then fp16(. * scale): the two roundings of lm8_weights, bit for bit (-ffp-contract=off, Makefile).
//   x         staged once per workgroup in LDS, wave w rows w (and no other: M <= 16), so a row's RMSNorm statistic is one wave's sum -- no barrier
//             but the one behind the staging, and the same order whatever M: gamma * fp16(x * rsqrt(mean x^2 + eps)), the expression of
//             lm8_gemv_kernel<NORM>.  Row stride (K + 8) halves: the 16 columns of an operand read (ds_read_b128, lane r at r * stride) lie 16 bytes
//             apart modulo 256 -- all 64 banks once.  Lanes of columns >= M read a zeroed 256 bytes in front of the rows (their per-group address
//             increment is 0): zero in registers, nothing staged for them.
//   edges     rows of the last tile past N are clamped to row N - 1 for the loads and never stored.  y rows start at m N halves: a lane's four
//             values go out as one 8-byte store where the address allows, as four halves otherwise.
// Column m of the accumulator depends on row m of x and on W only, and the k order is fixed: row m of an M-row call equals the 1-row call bit for bit.
// The summation order differs from lm8_gemv_kernel's (a different last bit): the runner takes this kernel by option only.
// No inline assembly, no hand-counted wait: every wait is the compiler's.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int LG_WAVES = 16;
constexpr int LG_D = 4;                 // groups of 128 k per register buffer
constexpr unsigned LG_X0 = 256;         // bytes: the zero block in front of the staged rows
constexpr int LG_PAD = 8;               // halves behind every staged row

struct LgBuf { u4 c[LG_D][2]; uint32_t m[LG_D]; };

// the weights of 8 consecutive codes (two dwords) as one MFMA operand
__device__ __forceinline__ h8 lg_weights8(uint32_t w0, uint32_t w1, h2 z2, h2 s2) {
    const h2 k1024 = bcast((_Float16)1024.0f);
    const h2 a = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u)) - k1024) - z2) * s2;
    const h2 b = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u)) - k1024) - z2) * s2;
    const h2 c = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u)) - k1024) - z2) * s2;
    const h2 d = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u)) - k1024) - z2) * s2;
    return (h8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

}  // namespace

template <bool NORM>
__global__ __launch_bounds__(LG_WAVES * 64) void lm8_gemm_kernel(const _Float16* x, const uint8_t* codes, const uint32_t* meta, _Float16* y,
                                                                 const _Float16* gamma, float eps, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = K >> 3;
    const int stride = K + LG_PAD;                  // halves
    if (tid < 16) ((u4*)smem)[tid] = (u4){0u, 0u, 0u, 0u};
    if (wave < M) {                                 // wave w stages row w
        const _Float16* xm = x + (size_t)wave * K;
        _Float16* xlm = (_Float16*)(smem + LG_X0) + (size_t)wave * stride;
        if (!NORM) {
            for (int c = lane; c < chunks; c += 64) *(h8*)(xlm + 8 * c) = *(const h8*)(xm + 8 * c);
        } else {
            float ss = 0.f;
            for (int c = lane; c < chunks; c += 64) {
                const h8 v = *(const h8*)(xm + 8 * c);
                *(h8*)(xlm + 8 * c) = v;
#pragma unroll
                for (int i = 0; i < 8; ++i) { const float f = (float)v[i]; ss += f * f; }
            }
            const float rstd = rsqrtf(wave_sum_dpp(ss) / (float)K + eps);
            for (int c = lane; c < chunks; c += 64) {           // (each lane rewrites the chunks it wrote)
                const h8 v = *(h8*)(xlm + 8 * c);
                const h8 gm = *(const h8*)(gamma + 8 * c);
                h8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) { const _Float16 n = (_Float16)((float)v[i] * rstd); o[i] = gm[i] * n; }
                *(h8*)(xlm + 8 * c) = o;
            }
        }
    }
    __syncthreads();
    const int r = lane & 15, g = lane >> 4;
    const bool live = r < M;
    const unsigned xbase = (live ? LG_X0 + (unsigned)r * (unsigned)stride * 2u : 0u) + 32u * g;      // bytes; a dead lane stays inside the zero block
    const unsigned xinc = live ? 256u : 0u;
    const int G = K >> 7;
    const int tiles = (N + 15) >> 4;
    for (int t = blockIdx.x * LG_WAVES + wave; t < tiles; t += gridDim.x * LG_WAVES) {
        const int n = min(16 * t + r, N - 1);
        const uint8_t* cr = codes + (size_t)n * K + 16 * g;
        const uint32_t* mr = meta + (size_t)n * G;
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        auto load = [&](LgBuf& b, int q0) {         // unconditional: groups past the last are clamped to it (loaded again, not used)
#pragma unroll
            for (int u = 0; u < LG_D; ++u) {
                const int q = min(q0 + u, G - 1);
                b.c[u][0] = AMQ_STREAM_LOAD((const u4*)(cr + (size_t)q * 128));
                b.c[u][1] = AMQ_STREAM_LOAD((const u4*)(cr + (size_t)q * 128 + 64));
                b.m[u] = AMQ_STREAM_LOAD(mr + q);
            }
        };
        auto compute = [&](const LgBuf& b, int q0) {
#pragma unroll
            for (int u = 0; u < LG_D; ++u)
                if (q0 + u < G) {                   // (wave-uniform)
                    const unsigned char* xa = smem + xbase + (unsigned)(q0 + u) * xinc;
                    const h8 x0 = *(const h8*)xa, x1 = *(const h8*)(xa + 16), x2 = *(const h8*)(xa + 128), x3 = *(const h8*)(xa + 144);
                    const h2 sz = as_h2(b.m[u]);
                    const h2 s2 = bcast(sz[0]), z2 = bcast(sz[1]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lg_weights8(b.c[u][0].x, b.c[u][0].y, z2, s2), x0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lg_weights8(b.c[u][0].z, b.c[u][0].w, z2, s2), x1, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lg_weights8(b.c[u][1].x, b.c[u][1].y, z2, s2), x2, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lg_weights8(b.c[u][1].z, b.c[u][1].w, z2, s2), x3, acc, 0, 0, 0);
                }
        };
        LgBuf A, B;
        load(A, 0);
        for (int q0 = 0; q0 < G; q0 += 2 * LG_D) {
            load(B, q0 + LG_D);
            compute(A, q0);
            load(A, q0 + 2 * LG_D);
            compute(B, q0 + LG_D);
        }
        if (live) {
            const int n0 = 16 * t + 4 * g;
            _Float16* yp = y + (size_t)r * N + n0;
            if (n0 + 3 < N && ((size_t)yp & 7) == 0) {
                *(h4*)yp = (h4){(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n0 + i < N) yp[i] = (_Float16)acc[i];
            }
        }
    }
}

size_t lm8_gemm_lds_bytes(int M, int K) { return (size_t)LG_X0 + (size_t)M * (size_t)(K + LG_PAD) * 2; }

template <bool NORM>
static hipError_t launch_lm8_gemm_n(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K,
                                    hipStream_t st) {
    const size_t lds = lm8_gemm_lds_bytes(M, K);
    auto k = lm8_gemm_kernel<NORM>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int tiles = (N + 15) / 16;
    const int wgs = (tiles + LG_WAVES - 1) / LG_WAVES;
    hipLaunchKernelGGL(k, dim3(wgs < 256 ? wgs : 256), dim3(LG_WAVES * 64), lds, st, (const _Float16*)x, (const uint8_t*)codes,
                       (const uint32_t*)meta, (_Float16*)y, (const _Float16*)gamma, eps, M, N, K);
    return hipGetLastError();
}

// x: fp16 [M, K] contiguous, y: fp16 [M, N] contiguous, 1 <= M <= 16, K % 128 == 0, the rows fit LDS (checked by the caller: amq_capi.hip)
hipError_t launch_lm8_gemm(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K,
                           hipStream_t st) {
    StreamDevice sd_(st);                                  // kernel attributes are per device: the stream's, not the current one
    if (gamma) return launch_lm8_gemm_n<true>(x, codes, meta, y, gamma, eps, M, N, K, st);
    return launch_lm8_gemm_n<false>(x, codes, meta, y, nullptr, eps, M, N, K, st);
}

}  // namespace amq
