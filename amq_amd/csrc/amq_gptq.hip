// amq_gptq.hip -- fp16 W[N,K] + the upper Cholesky factor U[K,K] of the damped inverse Hessian -> HQQ Format A (W_q, scale, zero) and the rows'
// losses: GPTQ's error-feedback solve (asymmetric, grouped, no act-order, no static groups) in one fixed fp32 arithmetic.
//
// Three launches, no host read, no atomics, no synchronisation between workgroups (the rows of W are independent):
//   gptq_solve_kernel<G, BITS>  16 lanes own a row (4 rows per 64-lane wave, 4 waves = 16 rows per workgroup); a lane holds 8 consecutive columns of
//                               the row's current 128-column block in registers.  Per block: the block's fp16 values are read (W is read ONCE), every
//                               earlier column's error is subtracted in ascending column order (left-looking: e from the E trace, U's rows through
//                               double-buffered LDS tiles the workgroup's rows share; plain loads, compiler-counted waits), the groups' (s16, z)
//                               are fixed from those values, then the 128 columns are walked: the owner lane's value goes to the row's 16 lanes,
//                               all of them form q, w^ and e, and each subtracts e * U[i, j] from the columns j > i it holds.  Codes (one byte
//                               each) and errors go to the workspace, (s16, z) and the row's loss to the outputs.
//   quant_flag_kernel, quant_pack_kernel<BITS> (amq_quant_pack.hip): the waves' nonfinite flags ORed into the info block, the byte codes packed.
// Every operation is its own fp32 rounding (-ffp-contract=off, IEEE division, rintf) and every element receives its subtractions in ascending
// column order, so the result does not depend on the blocking: tests/gptq_solver_ref.py restates it in torch, bit for bit.
#include "amq_quant.cuh"

namespace amq {

// a thread's share of one tile -- UP 16-byte pieces of U's rows (Ut: the tile's first row at the block's first column; piece f is row f / 32,
// columns 4 * (f % 32) ...) -- and its row's errors of the tile's rows (Et), into registers
template <int UP, int EN, int THREADS>
__device__ __forceinline__ void gptq_fetch(f4 (&up)[UP], f4 (&en)[EN], const float* __restrict__ Ut, const float* __restrict__ Et, int K,
                                           int tid) {
#pragma unroll
    for (int k = 0; k < UP; ++k) {
        const int f = tid + THREADS * k;
        up[k] = *(const f4*)(Ut + (size_t)(f / (GPTQ_BLOCK / 4)) * K + 4 * (f % (GPTQ_BLOCK / 4)));
    }
#pragma unroll
    for (int k = 0; k < EN; ++k) en[k] = *(const f4*)(Et + 4 * k);
}

template <int G, int BITS>
__global__ __launch_bounds__(64 * GPTQ_WAVES) void gptq_solve_kernel(const _Float16* __restrict__ W, const float* __restrict__ U, int K,
                                                                     float* __restrict__ E, uint8_t* __restrict__ Q, _Float16* __restrict__ scale,
                                                                     _Float16* __restrict__ zero, float* __restrict__ row_loss,
                                                                     int* __restrict__ NF) {
    constexpr int L = GPTQ_LANES, C = GPTQ_BLOCK / GPTQ_LANES;      // 16 lanes x 8 columns
    constexpr int LG = G / C;                                       // lanes that hold one group
    constexpr int T = GPTQ_TILE, THREADS = 64 * GPTQ_WAVES;
    constexpr int UP = T * GPTQ_BLOCK / 4 / THREADS;                // 16-byte pieces of a U tile per thread
    constexpr float maxq = (float)((1 << BITS) - 1);
    static_assert(C == 8 && (G == 32 || G == 64 || G == 128) && T % 4 == 0 && GPTQ_BLOCK % T == 0 && UP * THREADS * 4 == T * GPTQ_BLOCK, "layout");
    __shared__ float utile[2][T * GPTQ_BLOCK];                      // T rows of U over the block's 128 columns, double-buffered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane & (L - 1);
    const size_t row = ((size_t)blockIdx.x * GPTQ_WAVES + wave) * (64 / L) + (lane / L);      // N % 16 == 0: every workgroup is full
    const size_t rowK = row * (size_t)K;
    float loss = 0.0f;
    bool bad = false;
    for (int i1 = 0; i1 < K; i1 += GPTQ_BLOCK) {
        const int col0 = i1 + lg * C;                               // this lane's first column
        float w[C];
        {
            const h8 v = *(const h8*)(W + rowK + col0);
#pragma unroll
            for (int c = 0; c < C; ++c) w[c] = (float)v[c];
        }
        // left-looking: the errors of all columns before the block, in ascending column order.  The workgroup's 16 rows need the same rows of U:
        // tiles of T rows go through LDS; while tile t is used, tile t + 1 and its rows' errors are on their way to registers.
        const int ntiles = i1 / T;                                  // (workgroup-uniform)
        f4 up[UP], en[T / 4];
        if (ntiles > 0) gptq_fetch<UP, T / 4, THREADS>(up, en, U + i1, E + rowK, K, tid);
        for (int t = 0; t < ntiles; ++t) {
            float* buf = utile[t & 1];
#pragma unroll
            for (int k = 0; k < UP; ++k) *(f4*)(buf + 4 * (tid + THREADS * k)) = up[k];
            float ev[T];
#pragma unroll
            for (int k = 0; k < T / 4; ++k) {
                ev[4 * k] = en[k].x;
                ev[4 * k + 1] = en[k].y;
                ev[4 * k + 2] = en[k].z;
                ev[4 * k + 3] = en[k].w;
            }
            __syncthreads();        // (one barrier per tile: buffer t & 1 is next written after the barrier of tile t + 1, which every wave reaches
                                    // only when it is done with tile t)
            if (t + 1 < ntiles) gptq_fetch<UP, T / 4, THREADS>(up, en, U + (size_t)(t + 1) * T * K + i1, E + rowK + (t + 1) * T, K, tid);
#pragma unroll
            for (int r = 0; r < T; ++r) {
                const float4 a = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C), b = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C + 4);
                const float uv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float p = ev[r] * uv[c];
                    w[c] = w[c] - p;
                }
            }
        }
        // group parameters from the block-start values
        float mn = w[0], mx = w[0];
#pragma unroll
        for (int c = 1; c < C; ++c) {
            mn = fminf(mn, w[c]);
            mx = fmaxf(mx, w[c]);
        }
#pragma unroll
        for (int m = 1; m < LG; m <<= 1) {
            mn = fminf(mn, __shfl_xor(mn, m));
            mx = fmaxf(mx, __shfl_xor(mx, m));
        }
        float xmin = fminf(mn, 0.0f), xmax = fmaxf(mx, 0.0f);
        if (xmin == 0.0f && xmax == 0.0f) {
            xmin = -1.0f;
            xmax = 1.0f;
        }
        const float s32 = (xmax - xmin) / maxq;
        const float s16 = fmaxf((float)(_Float16)s32, 0x1p-24f);
        const float z = rintf((-xmin) / s16);
        if ((lg & (LG - 1)) == 0) {
            const size_t r = row * (size_t)(K / G) + (size_t)(col0 / G);
            scale[r] = (_Float16)s16;
            zero[r] = (_Float16)z;
        }
        // the block's 128 columns: o = the lane of the row that holds column i, c = its register
        for (int o = 0; o < L; ++o) {
            const float so = __shfl(s16, o, L), zo = __shfl(z, o, L);
            float ev[C];
            Codes8 codes;
            const bool after = lg > o, from = lg >= o;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int gi = i1 + o * C + c;
                const float* u = U + (size_t)gi * K + col0;
                const float4 a = *(const float4*)u, b = *(const float4*)(u + 4);
                const float uv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                const float d = U[(size_t)gi * K + gi];
                const float wi = __shfl(w[c], o, L);
                const float q = fminf(fmaxf(rintf(wi / so) + zo, 0.0f), maxq);
                const float t = (q - zo) * so;
                const float wh = (float)(_Float16)t;
                const float r = wi - wh;
                const float e = r / d;
                const float r2 = r * r, d2 = d * d;
                loss = loss + (r2 / d2) / 2.0f;
                // (spelled out, not amq_quant.cuh's finite(): through the call the compiler schedules this loop 29 instructions longer, measured 9 % slower)
                bad = bad || !(fabsf(wi) < __builtin_inff()) || !(fabsf(e) < __builtin_inff()) || !(d > 0.0f && d < __builtin_inff());
                ev[c] = e;
                codes.put(c, q);
#pragma unroll
                for (int c2 = 0; c2 < C; ++c2) {
                    const float p = e * uv[c2];
                    const float nw = w[c2] - p;
                    w[c2] = (c2 > c ? from : after) ? nw : w[c2];
                }
            }
            if (lg == o) {
                *(float4*)(E + rowK + col0) = make_float4(ev[0], ev[1], ev[2], ev[3]);
                *(float4*)(E + rowK + col0 + 4) = make_float4(ev[4], ev[5], ev[6], ev[7]);
                codes.store(Q + rowK + col0);
            }
        }
        __syncthreads();        // the block's E is read by the row's other lanes in the next block
    }
    if (lg == 0) row_loss[row] = loss;
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) NF[blockIdx.x * GPTQ_WAVES + wave] = anybad ? 1 : 0;
}

hipError_t launch_gptq_quantize(const void* W, const void* U, int N, int K, int bits, int group, void* W_q, void* scale, void* zero,
                                void* row_loss, void* info, void* workspace, hipStream_t st) {
    const int wgs = gptq_workgroups(N), flags = gptq_flags(N);
    float* E = (float*)workspace;
    int* NF = (int*)(E + (size_t)N * K);
    uint8_t* Q = (uint8_t*)(NF + flags);
    if (hipError_t e = dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((gptq_solve_kernel<G(), B()>), dim3(wgs), dim3(64 * GPTQ_WAVES), 0, st, (const _Float16*)W, (const float*)U, K, E, Q,
                               (_Float16*)scale, (_Float16*)zero, (float*)row_loss, NF);
            return hipGetLastError();
        }))
        return e;
    if (hipError_t e = launch_quant_flags(NF, flags, (int*)info, st)) return e;
    return launch_pack_codes(Q, (size_t)N * K / group, group, bits, W_q, st);
}

}  // namespace amq
