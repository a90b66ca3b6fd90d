// amq_gptq.hip -- fp16 W[N,K] + the upper Cholesky factor U[K,K] of the damped inverse Hessian -> HQQ Format A (W_q, scale, zero) and the rows'
// losses: GPTQ's error-feedback solve (asymmetric, grouped, no act-order, no static groups) in one fixed fp32 arithmetic.
//
// Three launches, no host read, no atomics, no synchronisation between workgroups (the rows of W are independent):
//   solve_kernel<SOLVE_PLAIN, G, BITS> (amq_solve_body.cuh): the groups' (s16, z) are fixed from the block-start values and go to the outputs.
//   quant_flag_kernel, quant_pack_kernel<BITS> (amq_quant_pack.hip): the waves' nonfinite flags ORed into the info block, the byte codes packed.
// tests/gptq_solver_ref.py restates it in torch, bit for bit.
#include "amq_solve_body.cuh"

namespace amq {

hipError_t launch_gptq_quantize(const void* W, const void* U, int N, int K, int bits, int group, void* W_q, void* scale, void* zero,
                                void* row_loss, void* info, void* workspace, hipStream_t st) {
    return launch_solve(workspace, N, K, group, bits, W_q, info, st, [&](float* E, int* NF, uint8_t* Q) {
        return dispatch_group_bits(group, bits, [&](auto G, auto B) {
            hipLaunchKernelGGL((solve_kernel<SOLVE_PLAIN, G(), B()>), dim3(gptq_workgroups(N)), dim3(64 * GPTQ_WAVES), 0, st, (const _Float16*)W,
                               (const float*)U, K, E, Q, (_Float16*)scale, (_Float16*)zero, (float*)row_loss, NF, (const int*)nullptr, 0, 0, 0,
                               (_Float16*)nullptr, (int*)nullptr);
            return hipGetLastError();
        });
    });
}

}  // namespace amq
