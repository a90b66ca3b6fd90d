// 8-bit KV cache: int8 rows with one fp32 scale per (sequence, kv head, position), K and V separately.
//   kv8_store_kernel        the prompt pass' glue: rotated k / v rows -> codes and scales of cache rows pos0 .. pos0 + S - 1
//   attn_decode_kv8_kernel  one new token per sequence: rotate q / k, quantize and append the new row, attention over the DEQUANTIZED rows 0 .. pos
// The quantizer (kv8_quant16) is ONE function for both kernels: the appended bytes are the stored bytes.  Every operation of it is one
// individually rounded fp32 operation (-ffp-contract=off; division and rint correctly rounded), so tests/kv8_ref.py restates it bit for bit:
//   a = max |r_i|;  s = a / 127;  x_i = rint(r_i / s);  e_i = fma(-x_i, s, r_i);  c_i = clamp(x_i + (e_i > s / 2) - (e_i < -s / 2), -127, 127);
//   a == 0 -> s = 0, codes 0;  a row with inf / NaN -> s = NaN, codes 0.
// No hand-counted waits here: every wait is the compiler's.
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int KV8_D = 128;
constexpr int KV8_THREADS = 256;
constexpr int KV8_GROUPS = KV8_THREADS / 8;      // 8 lanes x 16 B = one 128-byte row: 32 rows per pass of the workgroup
constexpr int KV8_TILE = 256;                    // keys per online-softmax step
constexpr int KV8_RPT = KV8_TILE / KV8_GROUPS;   // rows of K and of V a group holds in registers per tile
constexpr int KV8_WS_STRIDE = KV8_D + 4;         // floats per (head, chunk): O[128], m, l, pad

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

// 16 codes -> 8 fp16 pairs (integers up to 127 are exact in fp16)
__device__ __forceinline__ void kv8_codes_h2(const u4& c, h2 (&o)[8]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int x = (int)c[w];
        o[2 * w] = (h2){(_Float16)(short)(signed char)(x & 0xFF), (_Float16)(short)(signed char)((x >> 8) & 0xFF)};
        o[2 * w + 1] = (h2){(_Float16)(short)(signed char)((x >> 16) & 0xFF), (_Float16)(short)(x >> 24)};
    }
}
__device__ __forceinline__ void kv8_codes_f32(const u4& c, float (&o)[16]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int x = (int)c[w];
        o[4 * w] = (float)(signed char)(x & 0xFF);
        o[4 * w + 1] = (float)(signed char)((x >> 8) & 0xFF);
        o[4 * w + 2] = (float)(signed char)((x >> 16) & 0xFF);
        o[4 * w + 3] = (float)(x >> 24);
    }
}

// units = rows * n_kv_heads * 2 (K, V); one 8-lane group per unit, 32 units per workgroup
__global__ __launch_bounds__(KV8_THREADS) void kv8_store_kernel(const _Float16* k, const _Float16* v, signed char* kc8, float* ksc, signed char* vc8,
                                                                 float* vsc, int pos0, int S, int nkv, int max_seq, long units) {
    const long u = (long)blockIdx.x * KV8_GROUPS + (threadIdx.x >> 3);
    if (u >= units) return;
    const int l8 = threadIdx.x & 7;
    const bool is_v = u & 1;
    const long rh = u >> 1;
    const long row = rh / nkv;
    const int kvh = (int)(rh - row * nkv);
    const long b = row / S;
    const int pos = pos0 + (int)(row - b * S);
    const _Float16* src = (is_v ? v : k) + ((size_t)row * nkv + kvh) * KV8_D + 16 * l8;
    const h8 r0 = *(const h8*)src, r1 = *(const h8*)(src + 8);
    float s;
    const u4 c = kv8_quant16(r0, r1, &s);
    const size_t crow = ((size_t)b * nkv + kvh) * (size_t)max_seq + (size_t)pos;
    *(u4*)((is_v ? vc8 : kc8) + crow * KV8_D + 16 * l8) = c;
    if (l8 == 0) (is_v ? vsc : ksc)[crow] = s;
}

struct Kv8Rest {
    void* out; const void* rope_table; int pos; float rope_theta;
    float* ws; int* tickets; int n_splits; int chunk; int hpw; int n_hblk;
};

// Grid (n_kv_heads * n_hblk, batch, n_splits).  A workgroup serves hpw <= HB query heads of ONE kv head over the keys [z chunk, (z + 1) chunk) from
// one read of the rows: groups of 8 lanes own rows t = tile + group + 32 i (16 bytes per lane: every wave-load is eight whole contiguous rows),
// all KV8_RPT K rows and V rows of a tile of 256 keys are requested before the first is used, each with its scale.  Per tile: scores of every
// head (v_dot2 on the codes as fp16 integers -- exact products, fp32 sums -- times the key's scale, times 1 / sqrt 128: fp32, never rounded to
// fp16), an online softmax in fp32 (running maximum m, sum l, accumulators rescaled by e^(m_old - m_new)), then acc += (p_t s_t) c_t with the V
// scale folded into the weight once per key.  Probabilities are NOT rounded to fp16.  The new token's row takes part in its DEQUANTIZED form,
// quantized here by every workgroup whose chunk holds it (same arithmetic, same bits) and appended by the group's first head block only.
// Several chunks: (O_z, m_z, l_z) into the workspace, a ticket per (sequence, kv head, head block), the last arriver combines in chunk order and
// resets the ticket.  Chunks wholly beyond the position leave at once (wave-uniform).
template <int HB>
__global__ __launch_bounds__(KV8_THREADS) void attn_decode_kv8_kernel(signed char* p_kc, float* p_ks, signed char* p_vc, float* p_vs, const void* p_state,
                                                                       int p_heads, int p_max_seq, const void* p_q, const void* p_k, const void* p_v,
                                                                       Kv8Rest rest) {
    __shared__ __attribute__((aligned(16))) _Float16 qs[HB][KV8_D];          // rotated q of the heads served
    __shared__ __attribute__((aligned(16))) _Float16 rk[KV8_D], rv[KV8_D];   // rotated new key, new value
    __shared__ __attribute__((aligned(16))) uint32_t nk[KV8_D / 4], nv[KV8_D / 4];   // ... as codes
    __shared__ float nsc[2];                                                 // ... and their scales
    __shared__ float sc[HB][KV8_TILE];                                       // scores, then p_t s_t
    __shared__ float vsl[KV8_TILE];                                          // V scales of the tile
    __shared__ float st_m[HB], st_l[HB], st_a[HB];
    __shared__ float part[HB][KV8_THREADS / 64][KV8_D];
    __shared__ int last_flag;
    const int tid = threadIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int n_heads = p_heads & 0xFF, n_kv_heads = (p_heads >> 8) & 0xFF, max_seq = p_max_seq;
    const bool cur_mode = (p_heads >> 16) & 1;
    int pos;
    if (cur_mode) pos = *(const int*)((const char*)p_state + 256);
    else if (p_state) pos = *(const int*)p_state;
    else pos = rest.pos;
    // a position outside the cache: nothing is written, every workgroup leaves, the step state's sticky error word is raised
    if (pos < 0 || pos >= max_seq) {
        if (cur_mode && tid == 0 && blockIdx.x == 0 && b == 0 && z == 0) *(int*)((char*)const_cast<void*>(p_state) + 260) = 1;
        return;
    }
    const int chunk = rest.chunk, c0 = z * chunk;
    if (c0 > pos) return;                               // a chunk wholly beyond the position
    const int n_act = pos / chunk + 1;
    const int t_end = min(pos + 1, c0 + chunk);
    const bool has_new = pos < c0 + chunk;
    const int G = n_heads / n_kv_heads, hpw = rest.hpw;
    const int kvh = blockIdx.x / rest.n_hblk, hb = blockIdx.x - kvh * rest.n_hblk;
    const int g0 = hb * hpw;                            // first head of the group served here
    const int nh_here = min(hpw, G - g0);
    const int h0 = kvh * G + g0;
    const int grp = tid >> 3, l8 = tid & 7, wave = tid >> 6, lane = tid & 63;
    const size_t cbase = ((size_t)b * n_kv_heads + kvh) * (size_t)max_seq;
    const signed char* const kc = p_kc + cbase * KV8_D;
    const signed char* const vc = p_vc + cbase * KV8_D;
    const float* const ksc = p_ks + cbase;
    const float* const vsc = p_vs + cbase;

    // The first tile's rows (and their scales) are requested HERE, in front of the rotation and the quantization of the new row: a workgroup of a
    // short chunk would otherwise start its only stream after two barriers and ~16 fp32 divisions per lane
    const int last_old = pos > 0 ? pos - 1 : 0;         // cache rows >= pos are never used (row pos is in flight: it comes from LDS)
    u4 kraw[KV8_RPT], vraw[KV8_RPT];
    float kscl[KV8_RPT], vscl[KV8_RPT];
    auto load_tile = [&](int t0) {
#pragma unroll
        for (int i = 0; i < KV8_RPT; ++i) {
            if (t0 + KV8_GROUPS * i < t_end) {          // wave-uniform: passes wholly past the context request nothing
                int t = t0 + grp + KV8_GROUPS * i;
                t = t < last_old ? t : last_old;
                kraw[i] = __builtin_nontemporal_load((const u4*)(kc + (size_t)t * KV8_D + 16 * l8));
                kscl[i] = ksc[t];
            }
        }
#pragma unroll
        for (int i = 0; i < KV8_RPT; ++i) {
            if (t0 + KV8_GROUPS * i < t_end) {
                int t = t0 + grp + KV8_GROUPS * i;
                t = t < last_old ? t : last_old;
                vraw[i] = __builtin_nontemporal_load((const u4*)(vc + (size_t)t * KV8_D + 16 * l8));
                vscl[i] = vsc[t];
            }
        }
    };
    load_tile(c0);

    // ---- rotation (the fp16 expression of the fp16 kernels), quantization and append of the new row
    {
        const int i = lane;                             // rotary pair (i, i + 64)
        _Float16 c16, s16;
        if (cur_mode) { const h2 cs = ((const h2*)p_state)[i]; c16 = cs.x; s16 = cs.y; }
        else if (rest.rope_table) { const h2 cs = ((const h2*)rest.rope_table)[(size_t)pos * 64 + i]; c16 = cs.x; s16 = cs.y; }
        else {                                          // LlamaRotaryEmbedding: 1 / base^(2i/d), fp32 (amq_decode.hip: rope_cs)
            const float inv_freq = 1.0f / powf(rest.rope_theta, (float)(2 * i) / (float)KV8_D);
            float sn, cs;
            sincosf((float)pos * inv_freq, &sn, &cs);
            c16 = (_Float16)cs;
            s16 = (_Float16)sn;
        }
        for (int j = wave; j < nh_here; j += KV8_THREADS / 64) {
            const _Float16* q = (const _Float16*)p_q + ((size_t)b * n_heads + h0 + j) * KV8_D;
            const _Float16 q0 = q[i], q1 = q[i + 64];
            qs[j][i] = q0 * c16 + (-q1) * s16;
            qs[j][i + 64] = q1 * c16 + q0 * s16;
        }
        if (has_new && wave == (KV8_THREADS / 64 - 1)) {
            const _Float16* kn = (const _Float16*)p_k + ((size_t)b * n_kv_heads + kvh) * KV8_D;
            const _Float16* vn = (const _Float16*)p_v + ((size_t)b * n_kv_heads + kvh) * KV8_D;
            const _Float16 k0 = kn[i], k1 = kn[i + 64];
            rk[i] = k0 * c16 + (-k1) * s16;
            rk[i + 64] = k1 * c16 + k0 * s16;
            rv[i] = vn[i];
            rv[i + 64] = vn[i + 64];
        }
    }
    if (tid < HB) { st_m[tid] = -INFINITY; st_l[tid] = 0.f; }
    __syncthreads();
    if (has_new && tid < 16) {                          // group 0: the key, group 1: the value
        const bool is_v = tid >> 3;
        const _Float16* src = (is_v ? rv : rk) + 16 * l8;
        float s;
        const u4 c = kv8_quant16(*(const h8*)src, *(const h8*)(src + 8), &s);
        *(u4*)((is_v ? nv : nk) + 4 * l8) = c;
        if (l8 == 0) nsc[is_v] = s;
        if (hb == 0) {                                  // exactly one workgroup per (sequence, kv head) appends
            *(u4*)((is_v ? p_vc : p_kc) + (cbase + (size_t)pos) * KV8_D + 16 * l8) = c;
            if (l8 == 0) (is_v ? p_vs : p_ks)[cbase + (size_t)pos] = s;
        }
    }
    __syncthreads();

    const float scale = 0.08838834764831845f;           // RN32(1 / sqrt 128) = 0x3DB504F3
    float acc[HB][16];
#pragma unroll
    for (int j = 0; j < HB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const u4 knew = *(const u4*)(nk + 4 * l8), vnew = *(const u4*)(nv + 4 * l8);
    const float ksnew = nsc[0], vsnew = nsc[1];

    for (int t0 = c0; t0 < t_end; t0 += KV8_TILE) {
        if (t0 != c0) load_tile(t0);
        // scores
#pragma unroll
        for (int i = 0; i < KV8_RPT; ++i) {
            const int x = grp + KV8_GROUPS * i, t = t0 + x;
            if (t0 + KV8_GROUPS * i < t_end) {
                const bool is_new = t == pos;
                u4 kr = kraw[i];
                float ksv = kscl[i];
                if (is_new) { kr = knew; ksv = ksnew; }
                h2 kh[8];
                kv8_codes_h2(kr, kh);
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    if (j < nh_here) {
                        const h8 qa = *(const h8*)(&qs[j][16 * l8]), qb = *(const h8*)(&qs[j][16 * l8 + 8]);
                        float s = 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_fdot2((h2){qa[2 * e], qa[2 * e + 1]}, kh[e], s, false);
#pragma unroll
                        for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_fdot2((h2){qb[2 * e], qb[2 * e + 1]}, kh[4 + e], s, false);
                        s = row8_sum(s);
                        if (l8 == 0) sc[j][x] = t < t_end ? (s * ksv) * scale : -INFINITY;
                    }
                }
                if (l8 == 0) vsl[x] = t < t_end ? (is_new ? vsnew : vscl[i]) : 0.f;
            } else if (l8 == 0) {
#pragma unroll
                for (int j = 0; j < HB; ++j) sc[j][x] = -INFINITY;
                vsl[x] = 0.f;
            }
        }
        __syncthreads();
        // online softmax: one wave per head
        for (int j = wave; j < nh_here; j += KV8_THREADS / 64) {
            float sv[KV8_TILE / 64];
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < KV8_TILE / 64; ++r) { sv[r] = sc[j][lane + 64 * r]; tmax = fmaxf(tmax, sv[r]); }
            tmax = wave_max_dpp(tmax);
            const float m_old = st_m[j], m_new = fmaxf(m_old, tmax);
            float lsum = 0.f;
#pragma unroll
            for (int r = 0; r < KV8_TILE / 64; ++r) {
                const float p = sv[r] == -INFINITY ? 0.f : __expf(sv[r] - m_new);
                lsum += p;
                sc[j][lane + 64 * r] = p == 0.f ? 0.f : p * vsl[lane + 64 * r];
            }
            lsum = wave_sum_dpp(lsum);
            if (lane == 0) {
                const float al = m_old == -INFINITY ? 0.f : __expf(m_old - m_new);
                st_a[j] = al;
                st_l[j] = st_l[j] * al + lsum;
                st_m[j] = m_new;
            }
        }
        __syncthreads();
        // acc = acc e^(m_old - m_new) + sum_t (p_t s_t) c_t
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            if (j < nh_here) {
                const float al = st_a[j];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] *= al;
            }
        }
#pragma unroll
        for (int i = 0; i < KV8_RPT; ++i) {
            const int x = grp + KV8_GROUPS * i, t = t0 + x;
            if (t0 + KV8_GROUPS * i < t_end) {
                u4 vr = vraw[i];
                if (t == pos) vr = vnew;
                float cf[16];
                kv8_codes_f32(vr, cf);
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    if (j < nh_here) {
                        const float w = sc[j][x];
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[j][e] = __builtin_fmaf(w, cf[e], acc[j][e]);
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- the 32 groups' accumulators: lanes of equal l8 within a wave (fixed tree), then the four waves in order
#pragma unroll
    for (int j = 0; j < HB; ++j) {
        if (j < nh_here) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float v = acc[j][e];
                v += __shfl_xor(v, 8);
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (lane < 8) part[j][wave][16 * l8 + e] = v;
            }
        }
    }
    __syncthreads();
    const bool single = n_act == 1;
    for (int j = tid >> 7; j < nh_here; j += KV8_THREADS / 128) {
        const int d = tid & 127;
        const float o = ((part[j][0][d] + part[j][1][d]) + part[j][2][d]) + part[j][3][d];
        const size_t hrow = (size_t)b * n_heads + h0 + j;
        if (single) {
            ((_Float16*)rest.out)[hrow * KV8_D + d] = (_Float16)(o / st_l[j]);
        } else {
            float* const w = rest.ws + (hrow * (size_t)rest.n_splits + z) * KV8_WS_STRIDE;
            __hip_atomic_store(w + d, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(w + KV8_D, st_m[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(w + KV8_D + 1, st_l[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (single) return;
    // publish: every thread releases its own stores at agent scope, the workgroup meets, ONE lane takes the ticket; the last arriver acquires
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int* const ticket = rest.tickets + ((size_t)b * n_kv_heads + kvh) * rest.n_hblk + hb;
        const int old = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == n_act - 1;
        if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every other chunk has taken its ticket: a replay finds zero
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag) return;
    __threadfence();
    // The combine's loads are issued side by side: every (m_c, l_c) pair of every head in ONE round trip into LDS (`part` is free by now), then the
    // O_c rows sixteen chunks at a time -- one dependent agent-scope load after the other costs an L2 round trip per chunk.  Chunk order throughout.
    float* const ml = &part[0][0][0];                   // [nh_here][n_act][2]
    const bool staged = 2 * nh_here * n_act <= HB * (KV8_THREADS / 64) * KV8_D;
    if (staged) {
        for (int i = tid; i < nh_here * n_act; i += KV8_THREADS) {
            const int j = i / n_act, c = i - j * n_act;
            const float* const wc = rest.ws + (((size_t)b * n_heads + h0 + j) * (size_t)rest.n_splits + c) * KV8_WS_STRIDE;
            ml[2 * i] = __hip_atomic_load(wc + KV8_D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ml[2 * i + 1] = __hip_atomic_load(wc + KV8_D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    for (int j = tid >> 7; j < nh_here; j += KV8_THREADS / 128) {
        const int d = tid & 127;
        const size_t hrow = (size_t)b * n_heads + h0 + j;
        const float* const w = rest.ws + hrow * (size_t)rest.n_splits * KV8_WS_STRIDE;
        const float* const mlj = ml + 2 * j * n_act;
        auto m_of = [&](int c) { return staged ? mlj[2 * c] : __hip_atomic_load(w + (size_t)c * KV8_WS_STRIDE + KV8_D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        auto l_of = [&](int c) { return staged ? mlj[2 * c + 1] : __hip_atomic_load(w + (size_t)c * KV8_WS_STRIDE + KV8_D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        float M = -INFINITY;
        for (int c = 0; c < n_act; ++c) M = fmaxf(M, m_of(c));
        float L = 0.f, O = 0.f;
        for (int c0b = 0; c0b < n_act; c0b += 16) {
            float ov[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int cc = c0b + i < n_act ? c0b + i : n_act - 1;
                ov[i] = __hip_atomic_load(w + (size_t)cc * KV8_WS_STRIDE + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (c0b + i < n_act) {                  // chunk order: deterministic whatever the arrival order
                    const float f = __expf(m_of(c0b + i) - M);
                    L += l_of(c0b + i) * f;
                    O += ov[i] * f;
                }
            }
        }
        ((_Float16*)rest.out)[hrow * KV8_D + d] = (_Float16)(O / L);
    }
}

template <int HB>
hipError_t launch_kv8_hb(const Kv8Args& a, int batch, int n_splits, void* ws, void* tickets, hipStream_t st) {
    const int G = a.n_heads / a.n_kv_heads;
    const int n_hblk = kv8_head_blocks(a.n_heads, a.n_kv_heads);
    const int hpw = (G + n_hblk - 1) / n_hblk;
    const int ns = n_splits < 1 ? 1 : n_splits;
    Kv8Rest rest{a.out, a.rope_table, a.pos, a.rope_theta, (float*)ws, (int*)tickets, ns, kv8_chunk(a.max_seq, ns), hpw, n_hblk};
    const void* state = a.step_state ? a.step_state : (const void*)a.pos_dev;
    const int heads = a.n_heads | (a.n_kv_heads << 8) | ((a.step_state ? 1 : 0) << 16);
    hipLaunchKernelGGL(attn_decode_kv8_kernel<HB>, dim3(a.n_kv_heads * n_hblk, batch, ns), dim3(KV8_THREADS), 0, st, (signed char*)a.kc8, (float*)a.ks,
                       (signed char*)a.vc8, (float*)a.vs, state, heads, a.max_seq, a.q, a.k, a.v, rest);
    return hipGetLastError();
}

}  // namespace

int kv8_head_blocks(int n_heads, int n_kv_heads) { return (n_heads / n_kv_heads + 7) / 8; }

int kv8_chunk(int max_seq, int n_splits) {
    const int c = (((max_seq + n_splits - 1) / n_splits) + 31) & ~31;
    return c < 32 ? 32 : c;
}

hipError_t launch_kv8_store(const void* k, const void* v, void* kc8, void* ks, void* vc8, void* vs, int pos0, int S, int batch, int n_kv_heads,
                            int max_seq, hipStream_t st) {
    const long units = (long)batch * S * n_kv_heads * 2;
    hipLaunchKernelGGL(kv8_store_kernel, dim3((unsigned)((units + KV8_GROUPS - 1) / KV8_GROUPS)), dim3(KV8_THREADS), 0, st, (const _Float16*)k,
                       (const _Float16*)v, (signed char*)kc8, (float*)ks, (signed char*)vc8, (float*)vs, pos0, S, n_kv_heads, max_seq, units);
    return hipGetLastError();
}

hipError_t launch_attn_decode_kv8(const Kv8Args& a, int batch, int n_splits, void* ws, void* tickets, hipStream_t st) {
    const int n_hblk = kv8_head_blocks(a.n_heads, a.n_kv_heads);
    const int hpw = (a.n_heads / a.n_kv_heads + n_hblk - 1) / n_hblk;
    if (hpw == 1) return launch_kv8_hb<1>(a, batch, n_splits, ws, tickets, st);
    if (hpw == 2) return launch_kv8_hb<2>(a, batch, n_splits, ws, tickets, st);
    if (hpw <= 4) return launch_kv8_hb<4>(a, batch, n_splits, ws, tickets, st);
    return launch_kv8_hb<8>(a, batch, n_splits, ws, tickets, st);
}

}  // namespace amq
