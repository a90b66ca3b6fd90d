// amq_gptq_static.hip -- GPTQ's solve with static groups and an activation order (gptq.py:230-242, 270-277, 304-305): fp16
// W[N,K] + a permutation perm[K] of its columns + the upper Cholesky factor U_p[K,K] of the damped inverse of the equally permuted Hessian -> HQQ
// Format A (W_q, scale, zero) in W's OWN column order and the rows' losses.  Every group's (s16, z) is fixed from the original, consecutive G
// columns before the solve; the solve walks the columns in perm's order and column perm[i] quantizes with the parameters of group perm[i] / G, so
// the result is an ordinary packed layer: nothing at inference time knows about the order.
//
// Four launches, no host read, no atomics, no synchronisation between workgroups:
//   gptq_static_params_kernel<G, BITS>  G / 8 lanes per (row, group), 8 fp16 values per lane: the plain solve's parameter arithmetic, applied once
//                                       to W as handed in.  Writes scale = s16 and zero = z, fp16 [R], Format A's group order.
//   solve_kernel<SOLVE_STATIC, G, BITS> (amq_solve_body.cuh): the lane's 8 values of a block are gathered from W[row, perm[col0 + c]] (W is still
//                                       read once) with their groups' (s16, z) as one packed word each; the byte code of walk column i goes to
//                                       Q[row, perm[i]], so the pack kernel reads original order.  The error trace E stays in walk order.
//   quant_flag_kernel, quant_pack_kernel<BITS> (amq_quant_pack.hip) end it.
// tests/gptq_static_ref.py restates it in torch, bit for bit.
#include "amq_solve_body.cuh"

namespace amq {

template <int G, int BITS>
__global__ __launch_bounds__(256) void gptq_static_params_kernel(const _Float16* __restrict__ W, size_t pieces, _Float16* __restrict__ scale,
                                                                 _Float16* __restrict__ zero) {
    constexpr int C = 8, LG = G / C;                                // lanes that hold one group (4, 8 or 16: a group never straddles a wave)
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
    float s16, z;
    gptq_group_params<BITS>(mn, mx, s16, z);
    if (gid < pieces && (gid & (LG - 1)) == 0) {
        scale[gid / LG] = (_Float16)s16;                            // W is row-major and G divides K: group gid / LG is row * (K / G) + col / G
        zero[gid / LG] = (_Float16)z;
    }
}

hipError_t launch_gptq_quantize_static(const void* W, const void* U, const void* perm, int N, int K, int bits, int group, void* W_q, void* scale,
                                       void* zero, void* row_loss, void* info, void* workspace, hipStream_t st) {
    const size_t pieces = (size_t)N * K / 8;
    return launch_solve(workspace, N, K, group, bits, W_q, info, st, [&](float* E, int* NF, uint8_t* Q) {
        return dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((gptq_static_params_kernel<G(), B()>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, (const _Float16*)W,
                               pieces, (_Float16*)scale, (_Float16*)zero);
            if (hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL((solve_kernel<SOLVE_STATIC, G(), B()>), dim3(gptq_workgroups(N)), dim3(64 * GPTQ_WAVES), 0, st, (const _Float16*)W,
                               (const float*)U, K, E, Q, (_Float16*)scale, (_Float16*)zero, (float*)row_loss, NF, (const int*)perm, 0, 0, 0,
                               (_Float16*)nullptr, (int*)nullptr);
            return hipGetLastError();
        });
    });
}

}  // namespace amq
