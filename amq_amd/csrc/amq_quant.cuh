// amq_quant.cuh -- what the device quantizers share (amq_quantize.hip, amq_awq.hip, amq_quant_pack.hip, and through amq_solve_body.cuh the three
// solves amq_gptq.hip, amq_gptq_static.hip, amq_owq.hip; no hot-path unit includes this): the Format A word, byte codes in pairs of words, the finite test and the bits x group dispatch of their launchers.  None of it rounds:
// the kernels' arithmetic stays where DESIGN.md 3.9 - 3.11 state it.  (The 8-column group extremes of the GPTQ solve and AWQ's round-to-nearest
// stay written out in both: as a shared function they rescheduled the solve)
#pragma once
#include <type_traits>

#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_inff(); }

// Format A (hqq/core/bitpack.py): the R rows of codes [R, G] are cut into C = 8 / BITS (3 bit: 10) chunks of `step` rows and chunk c goes to a fixed
// bit offset of every word [step, G], chunk 0 in the top bits; 3 bit: uint32 words, rows zero-padded to a multiple of 10; else bytes.
// One thread (of 256-thread workgroups) per word: stores the word of this thread, given code(row, col) -> the code of that element.
template <int BITS, typename F>
__device__ __forceinline__ void format_a_store(void* __restrict__ Wq, size_t R, int G, F code) {
    constexpr int C = BITS == 4 ? 2 : BITS == 2 ? 4 : 10;
    const size_t step = BITS == 3 ? (R + 9) / 10 : R / C;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= step * (size_t)G) return;
    const size_t row = gid / G;
    const int col = (int)(gid % G);
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const size_t r = (size_t)c * step + row;
        if (BITS == 3 && r >= R) continue;
        const int shift = BITS == 3 ? 27 - 3 * c : 8 - BITS * (c + 1);
        word |= (uint32_t)code(r, col) << shift;
    }
    if (BITS == 3) ((uint32_t*)Wq)[gid] = word;
    else ((uint8_t*)Wq)[gid] = (uint8_t)word;
}
// workgroups of a format_a_store launch
inline unsigned format_a_blocks(size_t R, int group, int bits) {
    const size_t words = (bits == 3 ? (R + 9) / 10 : R * bits / 8) * (size_t)group;
    return (unsigned)((words + 255) / 256);
}

// a lane's 8 codes, one byte each, as the two words it stores
struct Codes8 {
    uint32_t lo = 0, hi = 0;
    __device__ __forceinline__ void put(int c, float q) {
        const uint32_t qi = (uint32_t)q;
        if (c < 4) lo |= qi << (8 * c);
        else hi |= qi << (8 * (c - 4));
    }
    __device__ __forceinline__ void store(uint8_t* at) const { *(uint2*)at = make_uint2(lo, hi); }
};

// v among Vs: f(std::integral_constant<int, v>) -> its hipError_t; else hipErrorInvalidValue (a kernel that has no such instantiation)
template <int... Vs, typename F>
inline hipError_t dispatch(int v, F f) {
    hipError_t e = hipErrorInvalidValue;
    ((v == Vs ? (void)(e = f(std::integral_constant<int, Vs>{})) : (void)0), ...);
    return e;
}
template <typename F>
inline hipError_t dispatch_bits(int bits, F f) { return dispatch<2, 3, 4>(bits, f); }
// the GPTQ solve's and AWQ's kernels: groups that fit a 128-column block x bits
template <typename F>
inline hipError_t dispatch_group_bits(int group, int bits, F f) {
    return dispatch<32, 64, 128>(group, [&](auto G) { return dispatch_bits(bits, [&](auto B) { return f(G, B); }); });
}

}  // namespace amq
