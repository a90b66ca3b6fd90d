// amq_gptq_static.hip -- GPTQ's solve with static groups and an activation order (gptq.py:230-242, 270-277, 304-305): fp16
// W[N,K] + a permutation perm[K] of its columns + the upper Cholesky factor U_p[K,K] of the damped inverse of the equally permuted Hessian -> HQQ
// Format A (W_q, scale, zero) in W's OWN column order and the rows' losses.  Every group's (s16, z) is fixed from the original, consecutive G
// columns before the solve; the solve walks the columns in perm's order and column perm[i] quantizes with the parameters of group perm[i] / G, so
// the result is an ordinary packed layer: nothing at inference time knows about the order.  amq_gptq.hip (the plain solve) stays as it is.
//
// Four launches, no host read, no atomics, no synchronisation between workgroups:
//   gptq_static_params_kernel<G, BITS>  G / 8 lanes per (row, group), 8 fp16 values per lane: gptq_solve_kernel's parameter arithmetic, applied once
//                                       to W as handed in.  Writes scale = s16 and zero = z, fp16 [R], Format A's group order.
//   gptq_solve_static_kernel<G, BITS>   gptq_solve_kernel's shape (16 lanes own a row, 8 walk columns per lane, blocks of 128 walk columns, U's rows
//                                       through double-buffered LDS tiles) with four differences: the lane's 8 values of a block are gathered from
//                                       W[row, perm[col0 + c]] (W is still read once); at the block's start the lane loads the (s16, z) of its 8
//                                       columns' groups as one packed word each, and that word travels to the row's lanes beside the value (no
//                                       dependent global load in the serial walk); the byte code of walk column i goes to Q[row, perm[i]], so the
//                                       pack kernel reads original order; no parameters are derived here.  The error trace E stays in walk order.
//   quant_flag_kernel, quant_pack_kernel<BITS> (amq_quant_pack.hip) end it.
// Every operation is its own fp32 rounding (-ffp-contract=off, IEEE division, rintf) and every element receives its subtractions in ascending walk
// index: tests/gptq_static_ref.py restates it in torch, bit for bit.
#include "amq_quant.cuh"

namespace amq {

template <int G, int BITS>
__global__ __launch_bounds__(256) void gptq_static_params_kernel(const _Float16* __restrict__ W, size_t pieces, _Float16* __restrict__ scale,
                                                                 _Float16* __restrict__ zero) {
    constexpr int C = 8, LG = G / C;                                // lanes that hold one group (4, 8 or 16: a group never straddles a wave)
    constexpr float maxq = (float)((1 << BITS) - 1);
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;      // piece gid = the 8 values W[8 gid ...]; N * K / 8 is a multiple of 256
    const h8 v = *(const h8*)(W + 8 * (gid < pieces ? gid : 0));
    float mn = (float)v[0], mx = (float)v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) {
        mn = fminf(mn, (float)v[c]);
        mx = fmaxf(mx, (float)v[c]);
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
    if (gid < pieces && (gid & (LG - 1)) == 0) {
        scale[gid / LG] = (_Float16)s16;                            // W is row-major and G divides K: group gid / LG is row * (K / G) + col / G
        zero[gid / LG] = (_Float16)z;
    }
}

// a thread's share of one tile (gptq_fetch of amq_gptq.hip, which stays as it is)
template <int UP, int EN, int THREADS>
__device__ __forceinline__ void gptq_static_fetch(f4 (&up)[UP], f4 (&en)[EN], const float* __restrict__ Ut, const float* __restrict__ Et, int K,
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
__global__ __launch_bounds__(64 * GPTQ_WAVES) void gptq_solve_static_kernel(const _Float16* __restrict__ W, const float* __restrict__ U,
                                                                            const int* __restrict__ perm, int K, float* __restrict__ E,
                                                                            uint8_t* __restrict__ Q, const uint16_t* __restrict__ scale,
                                                                            const uint16_t* __restrict__ zero, float* __restrict__ row_loss,
                                                                            int* __restrict__ NF) {
    constexpr int L = GPTQ_LANES, C = GPTQ_BLOCK / GPTQ_LANES;      // 16 lanes x 8 walk columns
    constexpr int T = GPTQ_TILE, THREADS = 64 * GPTQ_WAVES;
    constexpr int UP = T * GPTQ_BLOCK / 4 / THREADS;                // 16-byte pieces of a U tile per thread
    constexpr float maxq = (float)((1 << BITS) - 1);
    static_assert(C == 8 && (G == 32 || G == 64 || G == 128) && T % 4 == 0 && GPTQ_BLOCK % T == 0 && UP * THREADS * 4 == T * GPTQ_BLOCK, "layout");
    __shared__ float utile[2][T * GPTQ_BLOCK];                      // T rows of U over the block's 128 walk columns, double-buffered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane & (L - 1);
    const size_t row = ((size_t)blockIdx.x * GPTQ_WAVES + wave) * (64 / L) + (lane / L);      // N % 16 == 0: every workgroup is full
    const size_t rowK = row * (size_t)K, rowG = row * (size_t)(K / G);
    float loss = 0.0f;
    bool bad = false;
    for (int i1 = 0; i1 < K; i1 += GPTQ_BLOCK) {
        const int col0 = i1 + lg * C;                               // this lane's first walk column
        // the original columns of the lane's 8 walk columns, their values and their groups' parameters (scale in the low half, zero in the high).
        // An entry outside 0..K-1 cannot be a permutation's: it is read as column 0 and sets the flag, so that nothing is touched out of bounds.
        float w[C];
        uint32_t sz[C];
        {
            const int4 a = *(const int4*)(perm + col0), b = *(const int4*)(perm + col0 + 4);
            const int pv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool in = (unsigned)pv[c] < (unsigned)K;
                bad = bad || !in;
                const int p = in ? pv[c] : 0;
                w[c] = (float)W[rowK + p];
                const size_t g = rowG + (size_t)(p / G);
                sz[c] = (uint32_t)scale[g] | ((uint32_t)zero[g] << 16);
            }
        }
        // left-looking: the errors of all walk columns before the block, in ascending walk index, through LDS tiles of T rows of U (as in
        // gptq_solve_kernel: while tile t is used, tile t + 1 and its rows' errors are on their way to registers)
        const int ntiles = i1 / T;                                  // (workgroup-uniform)
        f4 up[UP], en[T / 4];
        if (ntiles > 0) gptq_static_fetch<UP, T / 4, THREADS>(up, en, U + i1, E + rowK, K, tid);
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
            if (t + 1 < ntiles) gptq_static_fetch<UP, T / 4, THREADS>(up, en, U + (size_t)(t + 1) * T * K + i1, E + rowK + (t + 1) * T, K, tid);
#pragma unroll
            for (int r = 0; r < T; ++r) {
                const float4 a = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C), b = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C + 4);
                const float uv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float pr = ev[r] * uv[c];
                    w[c] = w[c] - pr;
                }
            }
        }
        // the block's 128 walk columns: o = the lane of the row that holds walk column i, c = its register
        for (int o = 0; o < L; ++o) {
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
                const uint32_t szo = __shfl(sz[c], o, L);
                const float so = (float)__builtin_bit_cast(_Float16, (uint16_t)(szo & 0xffffu));
                const float zo = (float)__builtin_bit_cast(_Float16, (uint16_t)(szo >> 16));
                const float q = fminf(fmaxf(rintf(wi / so) + zo, 0.0f), maxq);
                const float t = (q - zo) * so;
                const float wh = (float)(_Float16)t;
                const float r = wi - wh;
                const float e = r / d;
                const float r2 = r * r, d2 = d * d;
                loss = loss + (r2 / d2) / 2.0f;
                bad = bad || !(fabsf(wi) < __builtin_inff()) || !(fabsf(e) < __builtin_inff()) || !(d > 0.0f && d < __builtin_inff());
                ev[c] = e;
                codes.put(c, q);
#pragma unroll
                for (int c2 = 0; c2 < C; ++c2) {
                    const float pr = e * uv[c2];
                    const float nw = w[c2] - pr;
                    w[c2] = (c2 > c ? from : after) ? nw : w[c2];
                }
            }
            if (lg == o) {
                *(float4*)(E + rowK + col0) = make_float4(ev[0], ev[1], ev[2], ev[3]);
                *(float4*)(E + rowK + col0 + 4) = make_float4(ev[4], ev[5], ev[6], ev[7]);
                // (perm is read again, not kept in registers through the walk: the address of a store, off the walk's dependency chain)
                const int4 a = *(const int4*)(perm + col0), b = *(const int4*)(perm + col0 + 4);
                const int pv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int p = (unsigned)pv[c] < (unsigned)K ? pv[c] : 0;
                    Q[rowK + p] = (uint8_t)((c < 4 ? codes.lo : codes.hi) >> (8 * (c & 3)));
                }
            }
        }
        __syncthreads();        // the block's E is read by the row's other lanes in the next block
    }
    if (lg == 0) row_loss[row] = loss;
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) NF[blockIdx.x * GPTQ_WAVES + wave] = anybad ? 1 : 0;
}

hipError_t launch_gptq_quantize_static(const void* W, const void* U, const void* perm, int N, int K, int bits, int group, void* W_q, void* scale,
                                       void* zero, void* row_loss, void* info, void* workspace, hipStream_t st) {
    const int wgs = gptq_workgroups(N), flags = gptq_flags(N);
    const size_t pieces = (size_t)N * K / 8;
    float* E = (float*)workspace;
    int* NF = (int*)(E + (size_t)N * K);
    uint8_t* Q = (uint8_t*)(NF + flags);
    if (hipError_t e = dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((gptq_static_params_kernel<G(), B()>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, (const _Float16*)W,
                               pieces, (_Float16*)scale, (_Float16*)zero);
            if (hipError_t e2 = hipGetLastError()) return e2;
            hipLaunchKernelGGL((gptq_solve_static_kernel<G(), B()>), dim3(wgs), dim3(64 * GPTQ_WAVES), 0, st, (const _Float16*)W, (const float*)U,
                               (const int*)perm, K, E, Q, (const uint16_t*)scale, (const uint16_t*)zero, (float*)row_loss, NF);
            return hipGetLastError();
        }))
        return e;
    if (hipError_t e = launch_quant_flags(NF, flags, (int*)info, st)) return e;
    return launch_pack_codes(Q, (size_t)N * K / group, group, bits, W_q, st);
}

}  // namespace amq
