// amq_quant_pack.hip -- the two launches that end the GPTQ solve (amq_gptq.hip) and AWQ's passes (amq_awq.hip), DESIGN.md 3.9:
//   quant_flag_kernel        one workgroup: ORs the waves' nonfinite flags into the first word of the info block.
//   quant_pack_kernel<BITS>  one thread per Format A word (amq_quant.cuh format_a_store), from the byte codes [R, group] in the workspace.
// (HQQ's stop kernel ORs its flags itself and its emit kernel forms the codes it packs: amq_quantize.hip.)
#include "amq_quant.cuh"

namespace amq {

__global__ __launch_bounds__(256) void quant_flag_kernel(const int* __restrict__ NF, size_t n, int* __restrict__ info) {
    __shared__ int sbad[256];
    int bad = 0;
    for (size_t w = threadIdx.x; w < n; w += 256) bad |= NF[w];
    sbad[threadIdx.x] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any = 0;
        for (int j = 0; j < 256; ++j) any |= sbad[j];
        info[0] = any != 0;
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void quant_pack_kernel(const uint8_t* __restrict__ Q, size_t R, int G, void* __restrict__ Wq) {
    format_a_store<BITS>(Wq, R, G, [&](size_t r, int col) { return Q[r * G + col]; });
}

hipError_t launch_quant_flags(const int* NF, size_t n, int* info_word, hipStream_t st) {
    hipLaunchKernelGGL(quant_flag_kernel, dim3(1), dim3(256), 0, st, NF, n, info_word);
    return hipGetLastError();
}

hipError_t launch_pack_codes(const void* codes, size_t R, int group, int bits, void* W_q, hipStream_t st) {
    return dispatch_bits(bits, [&](auto B) {
        hipLaunchKernelGGL((quant_pack_kernel<B()>), dim3(format_a_blocks(R, group, bits)), dim3(256), 0, st, (const uint8_t*)codes, R, group, W_q);
        return hipGetLastError();
    });
}

}  // namespace amq
