// amq_lm8_gemm_rows.hip -- the 8-bit lm_head ("LM8") for many rows of x: y [M, N] = x [M, K] . W^T for any M >= 1 over the layer's
// bytes as amq_lm8.hip reads them (codes uint8 [N, K] row-major, meta fp16 [N, K / 128, 2]; no repacked copy, no workspace).  x arrives normed.
// lm8_gemm_kernel (amq_lm8_gemm.hip) keeps its <= 16 rows of x in LDS over the whole K and tiles only N; here a workgroup owns a BM x BN tile of y
// and walks K in groups of 128, so the layer is streamed once per BM rows of x and never written out as fp16.
//
//   tile      LR_BM = 128 rows of x by LR_BN = 256 vocabulary rows, 4 waves; wave w owns the 64 vocabulary rows 64 w .. 64 w + 63 of the tile (two
//             32-row A operands) against all 128 rows of x (four 32-column B operands): 2 x 4 accumulators of v_mfma_f32_32x32x16_f16 = 128 fp32
//             registers a lane, 64 MFMAs a group.  No split-K, no atomics, no cross-wave reduction: the same bits run to run.  Workgroup b has
//             M panel b / n_tiles and N tile b % n_tiles: the N tiles of one M panel run together and its K x 128 x 2 bytes of x (1 MB at
//             K = 4096) stay in L2 while they do.
//   weights   never in LDS.  Lane (r = lane % 32, h = lane / 32) loads, per group q and operand a, the 64 bytes 128 q + 64 h .. + 63 of the codes
//             of vocabulary row n0 + 64 w + 32 a + r as four 16-byte non-temporal loads, and the row's (scale, zero) dword of the group.  Piece j
//             (16 codes) is the lane's 8 k-slots of MFMA step 2 j (first 8 codes) and 2 j + 1 (last 8): k = 128 q + 64 h + 16 j + 8 e + 0 .. 7.
//             Two register buffers: the loads of group q + 1 are issued before the arithmetic of group q.
//   unpack    lm8_gemm_kernel's expression: v_perm_b32 puts a byte under 0x64 (the half 1024 + c), minus 1024 (exact), then fp16(c - zero), then
//             fp16(. * scale): the two roundings of lm8_weights, bit for bit (-ffp-contract=off, Makefile).
//   x         the 128 x 128 panel of the group goes global -> registers -> LDS once per workgroup (thread t: 16-byte pieces t + 256 i, i = 0 .. 7;
//             16 lanes = one 256-byte row), two LDS buffers, one barrier a group: the panel of group q + 1 is requested before the arithmetic of
//             group q and written behind it into the buffer group q - 1 was read from (every wave is past that barrier).  Both operands permute k
//             the same way: lane (c = lane % 32, h) reads for step 2 j + e the 16 bytes at 128 h + 32 j + 16 e of row 32 cb + c -- no transpose.
//             Row stride 272 bytes (128 halves + 8): the 16 lanes of one ds_read_b128 pass (c = 0 .. 15 or 16 .. 31, one h) lie 272 c = 16 c
//             modulo 256 bytes apart -- all 64 banks once, conflict-free; the staging writes of 16 lanes fill one row's 256 bytes, all banks once.
//             Rows of the last M panel past M are staged as zeros (their loads clamped to row M - 1, a select in front of the write): zero
//             operands, and no divergent branch in the loop.
//   edges     vocabulary rows past N are clamped to N - 1 for the loads and never stored; x rows past M are never stored.  A lane ends with
//             y[m0 + 32 cb + c][n0 + 64 w + 32 a + 8 i + 4 h + 0 .. 3], i = 0 .. 3: one 8-byte store where the address allows (y rows are N
//             halves apart: an odd N leaves rows unaligned), four halves otherwise.
//   offsets   32-bit from the bases: M K halves of x and N K bytes of codes stay below 2^32 bytes (checked by the caller: amq_capi.hip).
// Column m of an accumulator depends on row m of x and on W only, and the k order is fixed: row m of an M-row call equals row m of any other call
// of this entry point bit for bit.  The order differs from lm8_gemv_kernel's and lm8_gemm_kernel's (a different last bit).
// No inline assembly, no hand-counted wait: every wait is the compiler's.
//
// Balance: a wave reads the whole x panel from LDS each group (32 ds_read_b128 = 32 KB) behind 64 MFMAs of 32 cycles: 4 waves move 128 KB per
// 2048 cycles = 64 bytes a clock of the CU's 128.  One 32-row operand a wave (BN = 128) would sit at the LDS limit; BM = 256 (256 accumulator
// registers) halves the passes over the layer at many rows and doubles the idle MFMA work below 128 rows.  Neither alternative was built and
// measured: this tile is the first design.  Measured with it (profiles/lm8_gemm_rows.json): 322 us per M panel at 128256 x 4096
// (1.6 TB/s on the codes) -- neither LDS nor the matrix cores bound it, it waits for its loads (one group in flight at one wave per SIMD).
// 137 VGPRs + 128 AGPRs, no scratch.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int LR_CB = 4;                // 32-column blocks of x rows a tile
constexpr int LR_BM = 32 * LR_CB;
constexpr int LR_WAVES = 4;
constexpr int LR_BN = 64 * LR_WAVES;
constexpr int LR_THREADS = 64 * LR_WAVES;
constexpr unsigned LR_ROW = 272;        // bytes: a staged row of 128 halves and its pad
constexpr unsigned LR_BUF = LR_BM * LR_ROW;
constexpr int LR_XP = LR_BM * 16 / LR_THREADS;      // 16-byte pieces of the x panel a thread stages
static_assert(LR_BM == LM8_ROWS_BM, "amq_kernels.h states the tile height");

struct LrW { u4 c[2][4]; uint32_t m[2]; };

__device__ __forceinline__ h8 lr_weights8(uint32_t w0, uint32_t w1, h2 z2, h2 s2) {
    const h2 k1024 = bcast((_Float16)1024.0f);
    const h2 a = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u)) - k1024) - z2) * s2;
    const h2 b = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u)) - k1024) - z2) * s2;
    const h2 c = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u)) - k1024) - z2) * s2;
    const h2 d = ((as_h2(__builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u)) - k1024) - z2) * s2;
    return (h8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

}  // namespace

__global__ __launch_bounds__(LR_THREADS) void lm8_gemm_rows_kernel(const _Float16* x, const uint8_t* codes, const uint32_t* meta, _Float16* y, int M,
                                                                   int N, int K, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = (blockIdx.x / n_tiles) * LR_BM, n0 = (blockIdx.x % n_tiles) * LR_BN;
    const int G = K >> 7;
    const int r = lane & 31, h = lane >> 5;

    // x staging: piece p = tid + 256 i is the 16 bytes 16 (p % 16) of row p / 16
    unsigned xsrc[LR_XP], xdst[LR_XP];
    bool xlive[LR_XP];
#pragma unroll
    for (int i = 0; i < LR_XP; ++i) {
        const int p = tid + LR_THREADS * i, row = p >> 4, col = p & 15;
        xlive[i] = m0 + row < M;                    // a dead row is loaded from row M - 1 and staged as zeros: no branch in the loop
        xsrc[i] = ((unsigned)min(m0 + row, M - 1) * (unsigned)K + 8u * col) * 2u;      // bytes from x
        xdst[i] = (unsigned)row * LR_ROW + 16u * col;
    }
    auto xload = [&](u4 (&xr)[LR_XP], int q) {
#pragma unroll
        for (int i = 0; i < LR_XP; ++i) xr[i] = *(const u4*)((const unsigned char*)x + xsrc[i] + 256u * (unsigned)q);
    };
    auto xstore = [&](const u4 (&xr)[LR_XP], int q) {
#pragma unroll
        for (int i = 0; i < LR_XP; ++i) *(u4*)(smem + (q & 1) * LR_BUF + xdst[i]) = xlive[i] ? xr[i] : (u4){0u, 0u, 0u, 0u};
    };

    // weights: this lane's two vocabulary rows (clamped), its 64-byte half of every group
    unsigned coff[2], moff[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int n = min(n0 + 64 * wave + 32 * a + r, N - 1);
        coff[a] = (unsigned)n * (unsigned)K + 64u * h;
        moff[a] = (unsigned)n * (unsigned)G;
    }
    auto wload = [&](LrW& b, int q) {               // unconditional: a group past the last is clamped to it (loaded again, not used)
        const unsigned qq = (unsigned)min(q, G - 1);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int j = 0; j < 4; ++j) b.c[a][j] = AMQ_STREAM_LOAD((const u4*)(codes + coff[a] + 128u * qq + 16u * j));
            b.m[a] = AMQ_STREAM_LOAD(meta + moff[a] + qq);
        }
    };

    f16v acc[2][LR_CB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int cb = 0; cb < LR_CB; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][cb][i] = 0.f;

    const unsigned xrd = (unsigned)r * LR_ROW + 128u * h;          // this lane's operand bytes in column block 0
    auto compute = [&](const LrW& b, int q) {
        const unsigned char* xb = smem + (q & 1) * LR_BUF + xrd;
        h2 s2[2], z2[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) { const h2 sz = as_h2(b.m[a]); s2[a] = bcast(sz[0]); z2[a] = bcast(sz[1]); }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                h8 wa[2];
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    wa[a] = e == 0 ? lr_weights8(b.c[a][j].x, b.c[a][j].y, z2[a], s2[a]) : lr_weights8(b.c[a][j].z, b.c[a][j].w, z2[a], s2[a]);
#pragma unroll
                for (int cb = 0; cb < LR_CB; ++cb) {
                    const h8 xv = *(const h8*)(xb + cb * (32u * LR_ROW) + 32u * j + 16u * e);
                    acc[0][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[0], xv, acc[0][cb], 0, 0, 0);
                    acc[1][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[1], xv, acc[1][cb], 0, 0, 0);
                }
            }
        }
    };

    LrW cur, nxt;
    u4 xr[LR_XP];
    xload(xr, 0);
    wload(cur, 0);
    xstore(xr, 0);
    __syncthreads();
    for (int q = 0; q < G; ++q) {                   // (G, and so the branch around the staging, is uniform over the workgroup)
        const bool more = q + 1 < G;
        if (more) xload(xr, q + 1);
        wload(nxt, q + 1);
        compute(cur, q);
        if (more) xstore(xr, q + 1);
        __syncthreads();
        cur = nxt;
    }

#pragma unroll
    for (int cb = 0; cb < LR_CB; ++cb) {
        const int m = m0 + 32 * cb + r;
        if (m >= M) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int nb = n0 + 64 * wave + 32 * a + 8 * i + 4 * h;
                if (nb >= N) continue;
                _Float16* yp = y + (size_t)m * N + nb;
                const f16v& v = acc[a][cb];
                if (nb + 3 < N && ((size_t)yp & 7) == 0) {
                    *(h4*)yp = (h4){(_Float16)v[4 * i], (_Float16)v[4 * i + 1], (_Float16)v[4 * i + 2], (_Float16)v[4 * i + 3]};
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (nb + t < N) yp[t] = (_Float16)v[4 * i + t];
                }
            }
        }
    }
}

// x: fp16 [M, K] contiguous and normed, y: fp16 [M, N] contiguous, K % 128 == 0, M K halves and N K bytes below 2^32 bytes (the caller: amq_capi.hip)
hipError_t launch_lm8_gemm_rows(const void* x, const void* codes, const void* meta, void* y, int M, int N, int K, hipStream_t st) {
    StreamDevice sd_(st);                                  // kernel attributes are per device: the stream's, not the current one
    const size_t lds = 2 * (size_t)LR_BUF;
    auto k = lm8_gemm_rows_kernel;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const long long n_tiles = (N + LR_BN - 1) / LR_BN, m_panels = (M + LR_BM - 1) / LR_BM;
    hipLaunchKernelGGL(k, dim3((unsigned)(n_tiles * m_panels)), dim3(LR_THREADS), lds, st, (const _Float16*)x, (const uint8_t*)codes,
                       (const uint32_t*)meta, (_Float16*)y, M, N, K, (int)n_tiles);
    return hipGetLastError();
}

}  // namespace amq
