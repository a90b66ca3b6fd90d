// amq_awq.hip -- AWQ's two weight-side passes in one fixed fp32 arithmetic (include/amq_hip.h), ending in HQQ Format A.
//
//   awq_rtn_kernel<G, BITS>   fp16 W[N,K] (optionally times a column scale, optionally clamped to per-group bounds) -> round to nearest per group:
//                             byte codes, (s16, z) and / or the dense fake-quantized matrix (divided by the column scale again).  A thread holds 8
//                             consecutive columns, G / 8 lanes a group (its min and max by xor shuffles).  Then quant_flag_kernel ORs the waves'
//                             nonfinite flags into the info block and quant_pack_kernel turns the byte codes into Format A words (amq_quant_pack.hip).
//   awq_clip_kernel<G, BITS>  auto_clip_layer_asym's search on the matrix cores.  One wave owns 8 rows x one group.  The rows' 10 shrink steps are 80
//                             (row, step) pairs = 5 B tiles of v_mfma_f32_16x16x4_f32: lane (j = lane & 15, h = lane >> 4) of tile b builds, for
//                             pair 16 b + j, d[c] = w^_step[c] - w[c] of the columns c = 4 kk + h and keeps them in registers (G / 4 per tile).  X's
//                             rows pass in tiles of 16 as the A operand (fp16 in memory, widened on the way in; rows beyond T are zeros), G / 4
//                             MFMAs per B tile chain the group's columns in ascending order -- bit for bit an fmaf chain --, each lane squares its
//                             four outputs and adds them to its running sum, and at the end the four lane quarters are added as (0 + 1) + (2 + 3).
//                             The first strict minimum over the steps picks the bounds.
// No host read, no allocation, no atomics; every summation order depends on T only.  tests/awq_search_ref.py restates both in torch, bit for bit.
#include "amq_quant.cuh"

namespace amq {

// one group's parameters from its (clamped) extremes: s16 = fp16(max(xmax - xmin, 1e-5) / maxq), z = clamp(rint(-xmin / s16), 0, maxq) + 0
// (the addition turns the -0 that rint makes of a small positive xmin into +0: the stored zero has one bit pattern)
__device__ __forceinline__ void awq_group_params(float xmin, float xmax, float maxq, float& s16, float& z) {
    const float s = fmaxf(xmax - xmin, 1e-5f) / maxq;
    s16 = (float)(_Float16)s;
    z = fminf(fmaxf(rintf((-xmin) / s16), 0.0f), maxq) + 0.0f;
}

// q = clamp(rint(v / s16) + z, 0, maxq)
__device__ __forceinline__ float awq_code(float v, float s16, float z, float maxq) { return fminf(fmaxf(rintf(v / s16) + z, 0.0f), maxq); }

// w^ = fp16((q - z) * s16): what amq_dequantize_hqq_f16 and the matmul kernels make of (q, s16, z)
__device__ __forceinline__ float awq_weight(float q, float s16, float z) {
    const float t = (q - z) * s16;
    return (float)(_Float16)t;
}

// fp16(p) of an fp32 PRODUCT p, as two roundings (fp32, then fp16).  The empty asm makes the compiler hold p in a register as an fp32 value:
// without it, it folds fp16(a * b) into v_fma_mixlo_f16 -- ONE rounding, which differs wherever the fp32 product lands on an fp16 midpoint
// (shrink factors like fp32(0.55) times an fp16 extreme do so in about 1 group of 50).
__device__ __forceinline__ float awq_fp16_of_product(float p) {
    asm("" : "+v"(p));
    return (float)(_Float16)p;
}

template <int G, int BITS>
__global__ __launch_bounds__(256) void awq_rtn_kernel(const _Float16* __restrict__ W, const float* __restrict__ CS, const _Float16* __restrict__ HI,
                                                      const _Float16* __restrict__ LO, int K, uint8_t* __restrict__ Q,
                                                      _Float16* __restrict__ scale, _Float16* __restrict__ zero, _Float16* __restrict__ dense,
                                                      int* __restrict__ NF) {
    constexpr int C = 8, LG = G / C;
    constexpr float maxq = (float)((1 << BITS) - 1);
    static_assert(G == 32 || G == 64 || G == 128, "group");
    const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * C;      // N * K % 2048 == 0: every workgroup is full
    const size_t grp = e0 / G;                                           // K % G == 0: [N, K / G] row-major
    const int col = (int)(e0 % (size_t)K);
    const h8 raw = *(const h8*)(W + e0);
    float cs[C], v[C];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = (float)raw[c];
        if (CS) {
            cs[c] = CS[col + c];
            v[c] = awq_fp16_of_product(v[c] * cs[c]);
        } else {
            cs[c] = 1.0f;
        }
        bad = bad || !finite(v[c]);
    }
    if (HI) {
        const float hi = (float)HI[grp], lo = (float)LO[grp];
        bad = bad || !finite(hi) || !finite(lo);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = fminf(fmaxf(v[c], lo), hi);
    }
    float mn = v[0], mx = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) {
        mn = fminf(mn, v[c]);
        mx = fmaxf(mx, v[c]);
    }
#pragma unroll
    for (int m = 1; m < LG; m <<= 1) {
        mn = fminf(mn, __shfl_xor(mn, m));
        mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    float s16, z;
    awq_group_params(mn, mx, maxq, s16, z);
    if (scale && (threadIdx.x & (LG - 1)) == 0) {
        scale[grp] = (_Float16)s16;
        zero[grp] = (_Float16)z;
    }
    Codes8 codes;
    h8 out;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float q = awq_code(v[c], s16, z, maxq);
        float wh = awq_weight(q, s16, z);
        if (CS) {
            const float d = wh / cs[c];
            wh = (float)(_Float16)d;
        }
        bad = bad || !finite(wh);
        out[c] = (_Float16)wh;
        codes.put(c, q);
    }
    if (Q) codes.store(Q + e0);
    if (dense) *(h8*)(dense + e0) = out;
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((threadIdx.x & 63) == 0) NF[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = anybad ? 1 : 0;
}

// the fp32 nearest to 1 - i / 20
__device__ __forceinline__ float awq_shrink(int i) { return (float)(1.0 - (double)i / 20.0); }

template <int G, int BITS>
__global__ __launch_bounds__(64) void awq_clip_kernel(const _Float16* __restrict__ W, const _Float16* __restrict__ X, int K, int T,
                                                      _Float16* __restrict__ HI, _Float16* __restrict__ LO, int* __restrict__ BEST,
                                                      float* __restrict__ ERR, int* __restrict__ NF) {
    constexpr int KS = G / 4, PAIRS = AWQ_ROWS * AWQ_STEPS;
    constexpr float maxq = (float)((1 << BITS) - 1);
    static_assert((G == 32 || G == 64 || G == 128) && PAIRS == 16 * AWQ_TILES, "layout");
    __shared__ float s_err[PAIRS], s_mx[AWQ_ROWS], s_mn[AWQ_ROWS];
    const int lane = threadIdx.x, j = lane & 15, h = lane >> 4;
    const int kg = K / G, g = (int)(blockIdx.x % (unsigned)kg);
    const size_t row0 = (size_t)(blockIdx.x / (unsigned)kg) * AWQ_ROWS;      // N % 8 == 0: every wave's rows exist
    const size_t cbase = (size_t)g * G + h;                                  // this lane's columns: cbase + 4 kk
    bool bad = false;
    // B: pair p = 16 b + j = (row p / 10, step p % 10); the lane keeps d[4 kk + h] of that pair
    float bd[AWQ_TILES][KS];
#pragma unroll
    for (int b = 0; b < AWQ_TILES; ++b) {
        const int p = 16 * b + j, r = p / AWQ_STEPS, i = p % AWQ_STEPS;
        const _Float16* wr = W + (row0 + r) * (size_t)K + cbase;
        float wv[KS];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            wv[kk] = (float)wr[4 * kk];
            bad = bad || !finite(wv[kk]);
        }
        float mn = wv[0], mx = wv[0];
#pragma unroll
        for (int kk = 1; kk < KS; ++kk) {
            mn = fminf(mn, wv[kk]);
            mx = fmaxf(mx, wv[kk]);
        }
        mn = fminf(mn, __shfl_xor(mn, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mn = fminf(mn, __shfl_xor(mn, 32));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (i == 0 && h == 0) {
            s_mx[r] = mx;
            s_mn[r] = mn;
        }
        const float f = awq_shrink(i);
        const float hi = awq_fp16_of_product(mx * f), lo = awq_fp16_of_product(mn * f);
        // (clamping is monotone: the clamped group's extremes are the clamped extremes)
        const float cmax = fminf(fmaxf(mx, lo), hi), cmin = fminf(fmaxf(mn, lo), hi);
        float s16, z;
        awq_group_params(cmin, cmax, maxq, s16, z);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const float vc = fminf(fmaxf(wv[kk], lo), hi);
            const float wh = awq_weight(awq_code(vc, s16, z, maxq), s16, z);
            bd[b][kk] = wh - wv[kk];
        }
    }
    float sq[AWQ_TILES];
#pragma unroll
    for (int b = 0; b < AWQ_TILES; ++b) sq[b] = 0.0f;
    const int tiles = (T + 15) / 16;
    for (int tt = 0; tt < tiles; ++tt) {
        // A: row 16 tt + j of X, column 4 kk + h of the group (rows beyond T: zeros, read from row 0's address and discarded)
        const int t = 16 * tt + j;
        const bool in = t < T;
        const _Float16* xr = X + (size_t)(in ? t : 0) * K + cbase;
        float xa[KS];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const float x = (float)xr[4 * kk];
            xa[kk] = in ? x : 0.0f;
        }
        f4 acc[AWQ_TILES];
#pragma unroll
        for (int b = 0; b < AWQ_TILES; ++b) acc[b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
            for (int b = 0; b < AWQ_TILES; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kk], bd[b][kk], acc[b], 0, 0, 0);
        }
        // C: column j = the pair, row 4 h + reg = the token inside the tile
#pragma unroll
        for (int b = 0; b < AWQ_TILES; ++b) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float o = acc[b][r];
                const float o2 = o * o;
                sq[b] = sq[b] + o2;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < AWQ_TILES; ++b) {
        const float a = sq[b] + __shfl_xor(sq[b], 16);       // quarters (0 + 1) and (2 + 3) ...
        const float e = a + __shfl_xor(a, 32);               // ... then their sum
        bad = bad || !finite(e);
        if (h == 0) s_err[16 * b + j] = e;
    }
    __syncthreads();
    const size_t out0 = row0 * (size_t)kg + (size_t)g;       // [N, K / G] index of the slab's first row
    for (int p = lane; p < PAIRS; p += 64) ERR[(out0 + (size_t)(p / AWQ_STEPS) * kg) * AWQ_STEPS + (p % AWQ_STEPS)] = s_err[p];
    if (lane < AWQ_ROWS) {
        int best = 0;
        float m = s_err[AWQ_STEPS * lane];
        for (int i = 1; i < AWQ_STEPS; ++i) {
            const float e = s_err[AWQ_STEPS * lane + i];
            if (e < m) {            // strict: the least shrink wins a tie
                m = e;
                best = i;
            }
        }
        const float f = awq_shrink(best);
        const size_t o = out0 + (size_t)lane * kg;
        HI[o] = (_Float16)awq_fp16_of_product(s_mx[lane] * f);
        LO[o] = (_Float16)awq_fp16_of_product(s_mn[lane] * f);
        BEST[o] = best;
    }
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) NF[blockIdx.x] = anybad ? 1 : 0;
}

hipError_t launch_awq_quantize(const void* W, const void* col_scale, const void* hi, const void* lo, int N, int K, int bits, int group, void* W_q,
                               void* scale, void* zero, void* dense, void* info, void* workspace, hipStream_t st) {
    const size_t flags = awq_quantize_flags(N, K);
    int* NF = (int*)workspace;
    uint8_t* Q = W_q ? (uint8_t*)(NF + flags) : nullptr;
    const unsigned wgs = (unsigned)((size_t)N * K / 2048);
    if (hipError_t e = dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((awq_rtn_kernel<G(), B()>), dim3(wgs), dim3(256), 0, st, (const _Float16*)W, (const float*)col_scale, (const _Float16*)hi,
                               (const _Float16*)lo, K, Q, (_Float16*)scale, (_Float16*)zero, (_Float16*)dense, NF);
            return hipGetLastError();
        }))
        return e;
    if (hipError_t e = launch_quant_flags(NF, flags, (int*)info, st)) return e;
    if (!W_q) return hipSuccess;
    return launch_pack_codes(Q, (size_t)N * K / group, group, bits, W_q, st);
}

hipError_t launch_awq_clip(const void* W, const void* X, int N, int K, int T, int bits, int group, void* hi, void* lo, void* best, void* err,
                           void* info, void* workspace, hipStream_t st) {
    if (T < 1 || group < 1) return hipErrorInvalidValue;
    const size_t waves = awq_clip_flags(N, K, group);
    int* NF = (int*)workspace;
    if (hipError_t e = dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((awq_clip_kernel<G(), B()>), dim3((unsigned)waves), dim3(64), 0, st, (const _Float16*)W, (const _Float16*)X, K, T,
                               (_Float16*)hi, (_Float16*)lo, (int*)best, (float*)err, NF);
            return hipGetLastError();
        }))
        return e;
    return launch_quant_flags(NF, waves, (int*)info, st);
}

}  // namespace amq
