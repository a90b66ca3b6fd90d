// amq_lm8.hip -- the 8-bit lm_head ("LM8"): codes uint8 [N, K] row-major, meta fp16 [N, K / 128, 2] = (scale, zero) per
// group of 128 along K (HQQ conventions: the stored scale is the multiplier, the zero is fractional).  The weight a layer stands for is
//
//     w = fp16(fp16(fp16(c) - zero) * scale)                    (two fp16 roundings, the reference's dequantize(); overflow to inf included)
//
//   lm8_gemv_kernel        y = (RMSNorm'ed) x . W^T for 1 .. 8 rows of x, W streamed once: the shape of gemv_f16w_kernel (amq_decode.hip) with
//                          16 codes instead of 8 halves behind every 16-byte load
//   lm8_dequantize_kernel  rows row0 .. row0 + rows - 1 of W as fp16 [rows, K]
//
// A byte becomes an fp16 integer exactly: the byte is placed in the low mantissa bits of 0x6400 (= 1024.0, whose ulp is 1), which gives
// 1024 + c, and 1024 is subtracted -- exact, as both are integers below 2048.  The zero is subtracted from THAT value in an operation of its own
// (one fp16 rounding of c - zero: no bias is folded into the zero), then the product with the scale is rounded.  -ffp-contract=off (Makefile)
// keeps the two operations apart.  No inline assembly, no hand-counted wait: every wait is the compiler's.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

// halves {c_lo, c_hi} of two bytes of w: B = 0 -> bytes 0, 1; B = 1 -> bytes 2, 3
template <int B>
__device__ __forceinline__ h2 lm8_pair(uint32_t w) {
    const uint32_t two = B == 0 ? ((w & 0xffu) | ((w & 0xff00u) << 8)) : (((w >> 16) & 0xffu) | ((w >> 8) & 0xff0000u));
    const h2 k1024 = {(_Float16)1024.0f, (_Float16)1024.0f};
    return as_h2(two | 0x64006400u) - k1024;
}

// the weights of one dword of codes: 4 halves in code order
__device__ __forceinline__ void lm8_weights(uint32_t w, h2 z, h2 s, h2& lo, h2& hi) {
    lo = (lm8_pair<0>(w) - z) * s;
    hi = (lm8_pair<1>(w) - z) * s;
}

__device__ __forceinline__ float lm8_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Where chunk c (the 8 halves x[8c .. 8c + 7]) of a staged row lies in LDS, in chunks.  A lane of the GEMV owns 16 consecutive k per wave-load of
// 1024: the two 16-byte halves of its x are kept 64 chunks apart, so that each of its two reads is one contiguous KiB across the wave (the rows
// as they lie would put the lanes 32 bytes apart: a two-way bank conflict on every read).  Rows are padded to whole wave-loads (lm8_kpad).
__device__ __forceinline__ int lm8_chunk(int c) { return (c & ~127) | ((c & 1) << 6) | ((c >> 1) & 63); }
static inline int lm8_kpad(int K) { return (K + 1023) & ~1023; }

// M = 1 .. 8 rows of x.  x (optionally RMSNorm'ed: gamma * fp16(x * rsqrt(mean x^2 + eps)), the expression of gemv_f16w_kernel<NORM>) staged in
// LDS; a wave owns PAIRS of adjacent rows of W (2 p, 2 p + 1: x is read from LDS once for both) and streams them 16 B = 16 codes per lane
// (1024 k per wave-load), four loads per row in flight (two at 6 - 7 rows of x, one at 8: the 128 registers of a 16-wave workgroup);
// the 16 codes of a lane lie inside one group: one (scale, zero) pair per lane and
// load.  A lane's sum over its k runs in the same order whatever M and WV are: rows of an M-row call equal single-row calls bit for bit.
template <bool NORM, int M, int WV>
__global__ __launch_bounds__(WV * 64) void lm8_gemv_kernel(const _Float16* x, const uint8_t* codes, const uint32_t* meta, _Float16* y,
                                                           const _Float16* gamma, float eps, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Kp = (K + 1023) & ~1023;
    _Float16* xl = (_Float16*)smem;                 // [M][Kp], chunks permuted (lm8_chunk)
    float* red = (float*)(smem + (size_t)M * Kp * 2);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = K >> 3;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const _Float16* xm = x + (size_t)m * K;
        _Float16* xlm = xl + (size_t)m * Kp;
        if (!NORM) {
            for (int c = tid; c < chunks; c += WV * 64) *(h8*)(xlm + 8 * lm8_chunk(c)) = *(const h8*)(xm + 8 * c);
        } else {
            float ss = 0.f;
            for (int c = tid; c < chunks; c += WV * 64) {
                h8 v = *(const h8*)(xm + 8 * c);
                *(h8*)(xlm + 8 * lm8_chunk(c)) = v;
#pragma unroll
                for (int i = 0; i < 8; ++i) { float f = (float)v[i]; ss += f * f; }
            }
            ss = lm8_wave_sum(ss);
            if (M > 1) __syncthreads();             // the previous row's readers of red[] are done
            if (lane == 0) red[wave] = ss;
            __syncthreads();
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < WV; ++w) tot += red[w];
            const float rstd = rsqrtf(tot / (float)K + eps);
            for (int c = tid; c < chunks; c += WV * 64) {       // (each thread rewrites the chunks it wrote)
                h8 v = *(h8*)(xlm + 8 * lm8_chunk(c));
                h8 g = *(const h8*)(gamma + 8 * c);
                h8 r;
#pragma unroll
                for (int i = 0; i < 8; ++i) { _Float16 n = (_Float16)((float)v[i] * rstd); r[i] = g[i] * n; }
                *(h8*)(xlm + 8 * lm8_chunk(c)) = r;
            }
        }
    }
    __syncthreads();
    const int gw = blockIdx.x * WV + wave, nw = gridDim.x * WV;
    const int steps = Kp >> 10;                     // 1024 k per wave-load; lanes past K are masked (K % 128 == 0: a lane's 16 codes are inside K or not)
    const int G = K >> 7;
    for (int pr = gw; 2 * pr < N; pr += nw) {
        const int row = 2 * pr;
        const bool two = row + 1 < N;               // (wave-uniform)
        const uint8_t* cr = codes + (size_t)row * K + 16 * lane;
        const uint32_t* mr = meta + (size_t)row * G + (lane >> 3);
        float acc[2][M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[0][m] = acc[1][m] = 0.f;
        constexpr int D = M <= 5 ? 4 : M <= 7 ? 2 : 1;  // loads per row in flight
        for (int s = 0; s < steps; s += D) {
            u4 buf[2][D];
            uint32_t mt[2][D];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < D; ++j)
                    if ((r == 0 || two) && s + j < steps && (s + j) * 1024 + 16 * lane < K) {
                        buf[r][j] = AMQ_STREAM_LOAD((const u4*)(cr + (size_t)r * K + (size_t)(s + j) * 1024));
                        mt[r][j] = AMQ_STREAM_LOAD(mr + (size_t)r * G + (s + j) * 8);
                    }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if (s + j < steps && (s + j) * 1024 + 16 * lane < K) {
                    h2 wt[2][8];                    // the 16 weights of the lane, both rows: unpacked once, used by every row of x
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        if (r == 0 || two) {
                            const h2 sz = as_h2(mt[r][j]);
                            const h2 s2 = {sz[0], sz[0]}, z2 = {sz[1], sz[1]};
                            const uint32_t cw[4] = {buf[r][j].x, buf[r][j].y, buf[r][j].z, buf[r][j].w};
#pragma unroll
                            for (int d = 0; d < 4; ++d) lm8_weights(cw[d], z2, s2, wt[r][2 * d], wt[r][2 * d + 1]);
                        }
                    }
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const h8 xa = *(const h8*)(xl + (size_t)m * Kp + (s + j) * 1024 + 8 * lane);
                        const h8 xb = *(const h8*)(xl + (size_t)m * Kp + (s + j) * 1024 + 512 + 8 * lane);
                        const h2 xp[8] = {{xa[0], xa[1]}, {xa[2], xa[3]}, {xa[4], xa[5]}, {xa[6], xa[7]},
                                          {xb[0], xb[1]}, {xb[2], xb[3]}, {xb[4], xb[5]}, {xb[6], xb[7]}};
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            if (r == 0 || two) {
#pragma unroll
                                for (int p = 0; p < 8; ++p) acc[r][m] = __builtin_amdgcn_fdot2(wt[r][p], xp[p], acc[r][m], false);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 0 || two) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float t = lm8_wave_sum(acc[r][m]);
                    if (lane == 0) y[(size_t)m * N + row + r] = (_Float16)t;
                }
            }
        }
    }
}

template <bool NORM, int M>
static hipError_t launch_lm8_gemv_m(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int N, int K,
                                    hipStream_t st) {
    const size_t lds = (size_t)M * lm8_kpad(K) * 2 + 64;
    constexpr int WV = M == 1 ? 4 : 16;             // as gemv_f16w_kernel: the staged x is what limits the workgroups per CU from 2 rows on
    auto k = lm8_gemv_kernel<NORM, M, WV>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(M == 1 ? 1024 : 512), dim3(WV * 64), lds, st, (const _Float16*)x, (const uint8_t*)codes, (const uint32_t*)meta,
                       (_Float16*)y, (const _Float16*)gamma, eps, N, K);
    return hipGetLastError();
}

template <bool NORM>
static hipError_t launch_lm8_gemv_n(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K,
                                    hipStream_t st) {
    switch (M) {
        case 1: return launch_lm8_gemv_m<NORM, 1>(x, codes, meta, y, gamma, eps, N, K, st);
        case 2: return launch_lm8_gemv_m<NORM, 2>(x, codes, meta, y, gamma, eps, N, K, st);
        case 3: return launch_lm8_gemv_m<NORM, 3>(x, codes, meta, y, gamma, eps, N, K, st);
        case 4: return launch_lm8_gemv_m<NORM, 4>(x, codes, meta, y, gamma, eps, N, K, st);
        case 5: return launch_lm8_gemv_m<NORM, 5>(x, codes, meta, y, gamma, eps, N, K, st);
        case 6: return launch_lm8_gemv_m<NORM, 6>(x, codes, meta, y, gamma, eps, N, K, st);
        case 7: return launch_lm8_gemv_m<NORM, 7>(x, codes, meta, y, gamma, eps, N, K, st);
        default: return launch_lm8_gemv_m<NORM, 8>(x, codes, meta, y, gamma, eps, N, K, st);
    }
}

size_t lm8_gemv_lds_bytes(int M, int K) { return (size_t)M * lm8_kpad(K) * 2 + 64; }

// x: fp16 [M, K] contiguous, y: fp16 [M, N] contiguous, 1 <= M <= 8, K % 128 == 0 (checked by the caller: amq_capi.hip)
hipError_t launch_lm8_gemv(const void* x, const void* codes, const void* meta, void* y, const void* gamma, float eps, int M, int N, int K,
                           hipStream_t st) {
    StreamDevice sd_(st);                                  // kernel attributes are per device: the stream's, not the current one
    if (gamma) return launch_lm8_gemv_n<true>(x, codes, meta, y, gamma, eps, M, N, K, st);
    return launch_lm8_gemv_n<false>(x, codes, meta, y, nullptr, eps, M, N, K, st);
}

// one thread per 16 codes (they share a group): out[(row - row0) * K + k], two 16-byte stores
__global__ __launch_bounds__(256) void lm8_dequantize_kernel(const uint8_t* codes, const uint32_t* meta, _Float16* out, int row0, long long pieces,
                                                             int K) {
    const int per_row = K >> 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (long long)gridDim.x * 256) {
        const long long r = i / per_row;
        const int k = (int)(i - r * per_row) << 4;
        const size_t row = (size_t)row0 + (size_t)r;
        const u4 c = *(const u4*)(codes + row * K + k);
        const h2 sz = as_h2(meta[row * (size_t)(K >> 7) + (k >> 7)]);
        const h2 s2 = {sz[0], sz[0]}, z2 = {sz[1], sz[1]};
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
        h8 o[2];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            h2 lo, hi;
            lm8_weights(cw[d], z2, s2, lo, hi);
            const int e = 4 * (d & 1);
            o[d >> 1][e] = lo[0]; o[d >> 1][e + 1] = lo[1]; o[d >> 1][e + 2] = hi[0]; o[d >> 1][e + 3] = hi[1];
        }
        _Float16* dst = out + (size_t)r * K + k;
        *(h8*)dst = o[0];
        *(h8*)(dst + 8) = o[1];
    }
}

hipError_t launch_lm8_dequantize(const void* codes, const void* meta, void* out, int row0, int rows, int K, hipStream_t st) {
    const long long pieces = (long long)rows * (K >> 4);
    const long long blocks = (pieces + 255) / 256;
    hipLaunchKernelGGL(lm8_dequantize_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, (const uint8_t*)codes,
                       (const uint32_t*)meta, (_Float16*)out, row0, pieces, K);
    return hipGetLastError();
}

}  // namespace amq
