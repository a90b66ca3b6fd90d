// amq_kv8.cuh -- the 8-bit KV cache's row quantizer, ONE function for every kernel that stores or appends a row
// (amq_attn_kv8.hip: kv8_store_kernel, attn_decode_kv8_kernel; amq_attn_kv8_gqa.hip: attn_decode_kv8_gqa_kernel): the appended bytes are the stored bytes.
// Every operation of it is one individually rounded fp32 operation (-ffp-contract=off; division and rint correctly rounded), so tests/kv8_ref.py
// restates it bit for bit:
//   a = max |r_i|;  s = a / 127;  x_i = rint(r_i / s);  e_i = fma(-x_i, s, r_i);  c_i = clamp(x_i + (e_i > s / 2) - (e_i < -s / 2), -127, 127);
//   a == 0 -> s = 0, codes 0;  a row with inf / NaN -> s = NaN, codes 0.
#pragma once
#include "amq_common.cuh"

namespace amq {

__device__ __forceinline__ float row8_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false)));
    return v;
}

// One row by the 8 lanes of a group: lane l holds elements 16 l .. 16 l + 15 (r0: the first eight, r1: the next).  Returns the lane's 16 codes
// (byte e of the 16 = element 16 l + e) and the row's scale in *scale (every lane of the group).  fmaxf drops a NaN, so a row that holds inf or
// NaN is flagged separately (|r| <= 65504 is false for both) and gets a NaN scale: it never comes out finite.
__device__ __forceinline__ u4 kv8_quant16(const h8& r0, const h8& r1, float* scale) {
    float r[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) { r[e] = (float)r0[e]; r[8 + e] = (float)r1[e]; }
    float a = 0.f, bad = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float m = fabsf(r[e]);
        a = fmaxf(a, m);
        bad = (m <= 65504.f) ? bad : 1.f;
    }
    a = row8_max(a);
    bad = row8_max(bad);
    const float s = a / 127.f, hs = 0.5f * s;
    const bool zero = (bad != 0.f) || (a == 0.f);
    u4 c;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ri = r[4 * w + e];
            float x = zero ? 0.f : rintf(ri / s);
            // the quotient near 127 is 2^-17 coarse: a value within that of a half step may have gone the wrong way.  One fma gives the
            // residual r - x s to fp32 accuracy; beyond half a step the code moves by one: |c s - r| <= s / 2 up to fp32 rounding
            const float res = __builtin_fmaf(-x, s, ri);
            x = zero ? 0.f : res > hs ? x + 1.f : res < -hs ? x - 1.f : x;
            x = fminf(fmaxf(x, -127.f), 127.f);
            word |= ((uint32_t)(int)x & 0xFFu) << (8 * e);
        }
        c[w] = word;
    }
    *scale = (bad != 0.f) ? __builtin_nanf("") : s;
    return c;
}

}  // namespace amq
