// amq_solve_body.cuh -- the error-feedback solve, once: the kernel body of the plain GPTQ solve (amq_gptq.hip), of the solve with static groups
// under an order (amq_gptq_static.hip) and of OWQ's solve (amq_owq.hip), and the launch tail the three share.
//
//   solve_kernel<V, G, BITS>  16 lanes own a row (4 rows per 64-lane wave, 4 waves = 16 rows per workgroup); a lane holds 8 consecutive walk columns
//                             of the row's current 128-column block in registers.  Per block: the lane's values are read (W is read ONCE), every
//                             earlier column's error is subtracted in ascending order (left-looking: e from the E trace, U's rows through
//                             double-buffered LDS tiles the workgroup's rows share; plain loads, compiler-counted waits), then the 128 columns are
//                             walked: the owner lane's value goes to the row's 16 lanes, all of them form q, w^ and e, and each subtracts
//                             e * U[i, j] from the columns j > i it holds.  Codes (one byte each) and errors go to the workspace, the row's loss to
//                             the output.
// The variants are compile-time arms of that ONE function body (`if constexpr (V == ...)`), not helper functions and not a shared body behind thin
// kernels: moved into a helper the tile phase reschedules, and behind a wrapper the kernel takes 276 VGPRs for 234 (one wave per SIMD for two).
//   SOLVE_PLAIN   the block's values are an h8 piece of W's row; the groups' (s16, z) are derived from the block-start values and written out.
//   SOLVE_STATIC  the block's values are gathered through perm, and with each the (scale, zero) of its column's group -- fixed before the solve by
//                 gptq_static_params_kernel -- as one packed word that travels to the row's lanes beside the value; the code of walk column i goes
//                 to Q[row, perm[i]].  No parameters are derived here.
//   SOLVE_OWQ     G = GPTQ_BLOCK.  Only the columns < nq are quantized: their group's (d16, zp) comes from the candidate search over the lane's 8
//                 registers + a 16-lane butterfly per candidate; the columns >= nq only receive the updates and leave as fp16 Wout.  E and Q rows
//                 are Kp long (nq padded to whole groups; the padding takes the code that dequantizes to 0).
// Every operation is its own fp32 rounding (-ffp-contract=off, IEEE division, rintf) and every element receives its subtractions in ascending walk
// index, so the result does not depend on the blocking: tests/gptq_solver_ref.py, tests/gptq_static_ref.py and tests/owq_ref.py restate the three
// in torch, bit for bit.
#pragma once
#include "amq_quant.cuh"

namespace amq {

enum { SOLVE_PLAIN, SOLVE_STATIC, SOLVE_OWQ };

// ---------------------------------------------------------------------------------------------------------------- OWQ's candidate arithmetic
// |d|^2.4 for the score: the hardware's log2 and exp2 (1 ulp each; d = 0 -> log2 = -inf -> 0; a denormal d counts as 0, its power underflows anyway)
__device__ __forceinline__ float owq_pow24(float d) { return __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf(d)); }

// candidate i's step: tmp_max = (xrange / num) * i, delta = max(tmp_max / maxq, 1e-8), d16 = max(fp16(delta), 2^-24)
__device__ __forceinline__ float owq_step(float xrange, float numf, int i, float maxq) {
    const float tmp_max = (xrange / numf) * (float)i;
    const float delta = fmaxf(tmp_max / maxq, 1e-8f);
    return fmaxf((float)(_Float16)delta, 0x1p-24f);
}

// the deployed weight of v's code under (d16, zp), given r = rint(v / d16)
template <int BITS>
__device__ __forceinline__ float owq_what(float r, float zp, float d16) {
    constexpr float maxq = (float)((1 << BITS) - 1);
    const float q = fminf(fmaxf(r + zp, 0.0f), maxq);
    const float t = (q - zp) * d16;
    return (float)(_Float16)t;
}

// ---------------------------------------------------------------------------------------------------------------- the solve
// a thread's share of one tile -- UP 16-byte pieces of U's rows (Ut: the tile's first row at the block's first column; piece f is row f / 32,
// columns 4 * (f % 32) ...) -- and its row's errors of the tile's rows (Et), into registers
template <int UP, int EN, int THREADS>
__device__ __forceinline__ void solve_fetch(f4 (&up)[UP], f4 (&en)[EN], const float* __restrict__ Ut, const float* __restrict__ Et, int K,
                                            int tid) {
#pragma unroll
    for (int k = 0; k < UP; ++k) {
        const int f = tid + THREADS * k;
        up[k] = *(const f4*)(Ut + (size_t)(f / (GPTQ_BLOCK / 4)) * K + 4 * (f % (GPTQ_BLOCK / 4)));
    }
#pragma unroll
    for (int k = 0; k < EN; ++k) en[k] = *(const f4*)(Et + 4 * k);
}

// a group's (s16, z) from the extremes of its values (the plain solve per block, gptq_static_params_kernel once): 0 is in the range, an all-zero
// group takes [-1, 1], the scale is rounded to fp16 before it is used and kept at or above 2^-24
template <int BITS>
__device__ __forceinline__ void gptq_group_params(float mn, float mx, float& s16, float& z) {
    constexpr float maxq = (float)((1 << BITS) - 1);
    float xmin = fminf(mn, 0.0f), xmax = fmaxf(mx, 0.0f);
    if (xmin == 0.0f && xmax == 0.0f) {
        xmin = -1.0f;
        xmax = 1.0f;
    }
    const float s32 = (xmax - xmin) / maxq;
    s16 = fmaxf((float)(_Float16)s32, 0x1p-24f);
    z = rintf((-xmin) / s16);
}

// One parameter list for the three: a variant's launcher passes null / 0 for what it does not use (perm: SOLVE_STATIC; nq, Kp, num, Wout, choice:
// SOLVE_OWQ).  scale / zero are written by SOLVE_PLAIN and SOLVE_OWQ and read by SOLVE_STATIC.
template <int V, int G, int BITS>
__global__ __launch_bounds__(64 * GPTQ_WAVES) void solve_kernel(const _Float16* __restrict__ W, const float* __restrict__ U, int K,
                                                                float* __restrict__ E, uint8_t* __restrict__ Q, _Float16* __restrict__ scale,
                                                                _Float16* __restrict__ zero, float* __restrict__ row_loss, int* __restrict__ NF,
                                                                const int* __restrict__ perm, int nq, int Kp, int num,
                                                                _Float16* __restrict__ Wout, int* __restrict__ choice) {
    constexpr int L = GPTQ_LANES, C = GPTQ_BLOCK / GPTQ_LANES;      // 16 lanes x 8 walk columns
    constexpr int LG = G / C;                                       // lanes that hold one group
    constexpr int T = GPTQ_TILE, THREADS = 64 * GPTQ_WAVES;
    constexpr int UP = T * GPTQ_BLOCK / 4 / THREADS;                // 16-byte pieces of a U tile per thread
    constexpr int NZ = 1 << BITS;
    constexpr float maxq = (float)(NZ - 1);
    static_assert(C == 8 && (G == 32 || G == 64 || G == 128) && T % 4 == 0 && GPTQ_BLOCK % T == 0 && UP * THREADS * 4 == T * GPTQ_BLOCK, "layout");
    static_assert(V == SOLVE_PLAIN || V == SOLVE_STATIC || (V == SOLVE_OWQ && G == GPTQ_BLOCK), "variant");
    __shared__ float utile[2][T * GPTQ_BLOCK];                      // T rows of U over the block's 128 walk columns, double-buffered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane & (L - 1);
    const size_t row = ((size_t)blockIdx.x * GPTQ_WAVES + wave) * (64 / L) + (lane / L);      // N % 16 == 0: every workgroup is full
    const size_t rowK = row * (size_t)K;                                                      // the row in W
    const size_t rowE = V == SOLVE_OWQ ? row * (size_t)Kp : rowK;                             // ... and in E and Q
    // (a variant's own values are formed here, ahead of the block loop, and only in that variant: inside the loop K is known to be positive and
    // K / G compiles to another sequence; formed in a variant that does not use them they reorder its prologue)
    [[maybe_unused]] const size_t rowG = V == SOLVE_STATIC ? row * (size_t)(K / G) : 0;       // SOLVE_STATIC: ... and in scale and zero
    [[maybe_unused]] const int n_out = V == SOLVE_OWQ ? K - nq : 0;
    [[maybe_unused]] const float numf = V == SOLVE_OWQ ? (float)num : 0.0f;
    float loss = 0.0f;
    bool bad = false;
    for (int i1 = 0; i1 < K; i1 += GPTQ_BLOCK) {
        const int col0 = i1 + lg * C;                               // this lane's first walk column
        float w[C];
        [[maybe_unused]] uint32_t sz[C];                            // SOLVE_STATIC: the columns' parameters, scale in the low half, zero in the high
        if constexpr (V == SOLVE_STATIC) {
            // the original columns of the lane's 8 walk columns, their values and their groups' parameters.  An entry outside 0..K-1 cannot be a
            // permutation's: it is read as column 0 and sets the flag, so that nothing is touched out of bounds.
            const uint16_t* sc = (const uint16_t*)scale;
            const uint16_t* zr = (const uint16_t*)zero;
            const int4 a = *(const int4*)(perm + col0), b = *(const int4*)(perm + col0 + 4);
            const int pv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool in = (unsigned)pv[c] < (unsigned)K;
                bad = bad || !in;
                const int p = in ? pv[c] : 0;
                w[c] = (float)W[rowK + p];
                const size_t g = rowG + (size_t)(p / G);
                sz[c] = (uint32_t)sc[g] | ((uint32_t)zr[g] << 16);
            }
        } else {
            const h8 v = *(const h8*)(W + rowK + col0);
#pragma unroll
            for (int c = 0; c < C; ++c) w[c] = (float)v[c];
        }
        // left-looking: the errors of all quantized walk columns before the block (SOLVE_OWQ: columns >= nq have none), in ascending order.  The
        // workgroup's 16 rows need the same rows of U: tiles of T rows go through LDS; while tile t is used, tile t + 1 and its rows' errors are on
        // their way to registers.  SOLVE_OWQ: ntiles * T <= i1 <= K and <= Kp: the last tile may reach past nq, its rows past nq are fetched and
        // skipped.
        const int prev = V == SOLVE_OWQ ? (i1 < nq ? i1 : nq) : i1;                           // (workgroup-uniform)
        const int ntiles = V == SOLVE_OWQ ? (prev + T - 1) / T : i1 / T;
        f4 up[UP], en[T / 4];
        if (ntiles > 0) solve_fetch<UP, T / 4, THREADS>(up, en, U + i1, E + rowE, K, tid);
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
            if (t + 1 < ntiles) solve_fetch<UP, T / 4, THREADS>(up, en, U + (size_t)(t + 1) * T * K + i1, E + rowE + (t + 1) * T, K, tid);
            const int rows = prev - t * T;                          // rows of this tile that are quantized columns (all T but for SOLVE_OWQ)
#pragma unroll
            for (int r = 0; r < T; ++r) {
                if (V != SOLVE_OWQ || r < rows) {
                    const float4 a = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C), b = *(const float4*)(buf + r * GPTQ_BLOCK + lg * C + 4);
                    const float uv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float p = ev[r] * uv[c];
                        w[c] = w[c] - p;
                    }
                }
            }
        }
        if (V != SOLVE_OWQ || i1 < nq) {
            float s16 = 0.0f, z = 0.0f;                             // the lane's group's parameters (SOLVE_STATIC: none, they travel in sz)
            if constexpr (V == SOLVE_PLAIN) {
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
                gptq_group_params<BITS>(mn, mx, s16, z);
                if ((lg & (LG - 1)) == 0) {
                    const size_t r = row * (size_t)(K / G) + (size_t)(col0 / G);
                    scale[r] = (_Float16)s16;
                    zero[r] = (_Float16)z;
                }
            }
            if constexpr (V == SOLVE_OWQ) {
                // the group's range from the row's current values of its columns < nq
                const int cnt = nq - i1 < GPTQ_BLOCK ? nq - i1 : GPTQ_BLOCK;
                const float cntf = (float)cnt;
                float mn = 0.0f, mx = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const bool in = col0 + c < nq;
                    mn = in ? fminf(mn, w[c]) : mn;
                    mx = in ? fmaxf(mx, w[c]) : mx;
                }
#pragma unroll
                for (int m = 1; m < L; m <<= 1) {
                    mn = fminf(mn, __shfl_xor(mn, m));
                    mx = fmaxf(mx, __shfl_xor(mx, m));
                }
                const float xrange = mx - mn;
                float best = 1e10f;
                int bi = 0;
#pragma unroll 1
                for (int i = 1; i <= num; ++i) {
                    const float d16 = owq_step(xrange, numf, i, maxq);
                    float r[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) r[c] = rintf(w[c] / d16);
                    // the sum's order: a lane adds its (up to) 8 columns in ascending order from 0, the row's 16 lanes meet in a butterfly (xor 1, 2,
                    // 4, 8); the score is that sum / the group's column count
#pragma unroll
                    for (int zi = 0; zi < NZ; ++zi) {
                        const float zp = (float)zi;
                        float s = 0.0f;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float term = owq_pow24(fabsf(w[c] - owq_what<BITS>(r[c], zp, d16)));
                            s = s + (col0 + c < nq ? term : 0.0f);
                        }
#pragma unroll
                        for (int m = 1; m < L; m <<= 1) s = s + __shfl_xor(s, m);
                        const float sc = s / cntf;
                        if (sc < best) {
                            best = sc;
                            s16 = d16;
                            z = zp;
                            bi = i;
                        }
                    }
                }
                bad = bad || bi == 0;                               // no winner: a non-finite value in the group
                if (lg == 0) {
                    const size_t g = row * (size_t)(Kp / GPTQ_BLOCK) + (size_t)(i1 / GPTQ_BLOCK);
                    scale[g] = (_Float16)s16;
                    zero[g] = (_Float16)z;
                    choice[2 * g] = bi;
                    choice[2 * g + 1] = (int)z;
                }
            }
            // the block's 128 walk columns: o = the lane of the row that holds walk column i, c = its register
            for (int o = 0; o < L; ++o) {
                float so = s16, zo = z;                             // column i's parameters (SOLVE_OWQ: the block's)
                if constexpr (V == SOLVE_PLAIN) {
                    so = __shfl(s16, o, L);
                    zo = __shfl(z, o, L);
                }
                float ev[C];
                Codes8 codes;
                const bool after = lg > o, from = lg >= o;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int gi = i1 + o * C + c;
                    if (V != SOLVE_OWQ || gi < nq) {                // (workgroup-uniform)
                        const float* u = U + (size_t)gi * K + col0;
                        const float4 a = *(const float4*)u, b = *(const float4*)(u + 4);
                        const float uv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                        const float d = U[(size_t)gi * K + gi];
                        const float wi = __shfl(w[c], o, L);
                        if constexpr (V == SOLVE_STATIC) {
                            const uint32_t szo = __shfl(sz[c], o, L);
                            so = (float)__builtin_bit_cast(_Float16, (uint16_t)(szo & 0xffffu));
                            zo = (float)__builtin_bit_cast(_Float16, (uint16_t)(szo >> 16));
                        }
                        const float q = fminf(fmaxf(rintf(wi / so) + zo, 0.0f), maxq);
                        const float t = (q - zo) * so;
                        const float wh = (float)(_Float16)t;
                        const float r = wi - wh;
                        const float e = r / d;
                        const float r2 = r * r, d2 = d * d;
                        loss = loss + (r2 / d2) / 2.0f;
                        // (spelled out, not amq_quant.cuh's finite(): through the call the compiler schedules this loop 29 instructions longer,
                        // measured 9 % slower)
                        bad = bad || !(fabsf(wi) < __builtin_inff()) || !(fabsf(e) < __builtin_inff()) || !(d > 0.0f && d < __builtin_inff());
                        ev[c] = e;
                        codes.put(c, q);
#pragma unroll
                        for (int c2 = 0; c2 < C; ++c2) {
                            const float p = e * uv[c2];
                            const float nw = w[c2] - p;
                            w[c2] = (c2 > c ? from : after) ? nw : w[c2];
                        }
                    } else {                                        // padding of a ragged last group: the code that dequantizes to 0
                        ev[c] = 0.0f;
                        codes.put(c, z);
                    }
                }
                if (lg == o) {
                    *(float4*)(E + rowE + col0) = make_float4(ev[0], ev[1], ev[2], ev[3]);
                    *(float4*)(E + rowE + col0 + 4) = make_float4(ev[4], ev[5], ev[6], ev[7]);
                    if constexpr (V == SOLVE_STATIC) {
                        // (perm is read again, not kept in registers through the walk: the address of a store, off the walk's dependency chain)
                        const int4 a = *(const int4*)(perm + col0), b = *(const int4*)(perm + col0 + 4);
                        const int pv[C] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const int p = (unsigned)pv[c] < (unsigned)K ? pv[c] : 0;
                            Q[rowK + p] = (uint8_t)((c < 4 ? codes.lo : codes.hi) >> (8 * (c & 3)));
                        }
                    } else {
                        codes.store(Q + rowE + col0);
                    }
                }
            }
        }
        if constexpr (V == SOLVE_OWQ) {
            // the columns >= nq this lane holds have all their updates now: they leave as fp16
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int j = col0 + c - nq;
                if (j >= 0) {
                    bad = bad || !(fabsf(w[c]) < __builtin_inff());
                    Wout[row * (size_t)n_out + j] = (_Float16)w[c];
                }
            }
        }
        __syncthreads();        // the block's E is read by the row's other lanes in the next block
    }
    if (lg == 0) row_loss[row] = loss;
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) NF[blockIdx.x * GPTQ_WAVES + wave] = anybad ? 1 : 0;
}

// The launch every solve shares, over its workspace of 5 N cols + 4 flags bytes: E [N, cols] fp32, the waves' flags NF, the byte codes Q [N, cols]
// are carved, solve(E, NF, Q) launches the variant, then the flags are ORed into the info word and the codes packed in groups of `group`.
template <typename F>
inline hipError_t launch_solve(void* workspace, int N, int cols, int group, int bits, void* W_q, void* info, hipStream_t st, F solve) {
    const int flags = gptq_flags(N);
    float* E = (float*)workspace;
    int* NF = (int*)(E + (size_t)N * cols);
    uint8_t* Q = (uint8_t*)(NF + flags);
    if (hipError_t e = solve(E, NF, Q)) return e;
    if (hipError_t e = launch_quant_flags(NF, flags, (int*)info, st)) return e;
    return launch_pack_codes(Q, (size_t)N * cols / group, group, bits, W_q, st);
}

}  // namespace amq
