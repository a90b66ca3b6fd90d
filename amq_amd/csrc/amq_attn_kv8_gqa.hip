// amq_attn_kv8_gqa.hip -- decode step of a GROUPED-QUERY model over the 8-bit KV cache on the matrix cores, gfx950.
//
// attn_decode_kv8_kernel (amq_attn_kv8.hip) repeats a v_dot2 score chain and an fp32 fma P.V chain once per query head on the vector units; here the
// G = n_heads / n_kv_heads (2 .. 16) rotated queries of a kv head are the rows of ONE 16-row MFMA block and a key row is scored against all of them
// by one instruction stream.  Grid (kv head, sequence, chunk), 256 threads; a chunk is `iters` stages of 128 keys.
//
//   staging   a stage = the RAW rows: 128 x 128 B of K codes, the same of V codes, 2 x 128 fp32 scales (33 KiB, half the fp16 kernel's stage), by
//             LDS-DMA into one of two buffers; stage it + 1 is in flight under stage it's arithmetic.  A DMA instruction moves 8 rows (lane l: row
//             l >> 3, 16-byte chunk l & 7); wave w moves pieces w, w + 4, w + 8, w + 12 of K and of V and one 64-key run of scales (4 bytes a lane).
//             LDS position p of row x holds chunk p ^ ((x >> 1) & 7) (applied on the source side): 16 rows x one chunk cover all 64 banks once, for
//             the K reads (ds_read_b128) and for the V reads (transposing, 8 rows x 16 bytes per 16 lanes).  Rows at or past the position are clamped
//             to the last cached row: nothing unwritten is read (codes are always finite as fp16; the scales of masked keys are SELECTED away).
//   scores    wave w takes keys 32 w .. 32 w + 31 of the stage.  S^T = K . Q^T on v_mfma_f32_16x16x32_f16: A = 16 key rows, codes turned into fp16
//             in registers (v_perm puts a byte under 0x64: 1024 + (c + 128), minus 1152 -- integers, exact), B = the lane's rotated q fragments.
//             The k-slots of step t in lane (r, o) are dims 64 (t >> 1) + 16 o + 8 (t & 1) + e: a lane's two 16-byte reads of a row feed four steps.
//             A lane then holds S^T[key 16 kl + 4 o + i][head r]; each is multiplied by the key's scale and by RN32(1 / sqrt 128) in fp32.
//   softmax   online, fp32, per wave: running maximum m (per head), sum l, accumulators rescaled by e^(m_old - m_new).
//   P.V       O^T = V^T . P^T.  B = the registers the softmax leaves (keys 16 kl + 4 o + i = k-slot 8 o + 4 kl + i), A = V^T through ds_read_b64_tr_b8
//             of the row-major int8 tile (8 rows x 16 bytes per 16 lanes -> lane r: byte r of each row), converted like K.  The V scale never enters
//             an fp16 quantity on its own: the weight is fp16(p_t (s_t / S)) with S the largest V scale of the wave's 32 keys (<= 1 times p_t <= 1),
//             the product T comes out of the MFMAs on a zero accumulator and O <- alpha O + S T in fp32.
//   new row   q and the new k rotated with the fp16 expression of every decode kernel; the workgroup whose chunk ends at the new token quantizes k / v
//             (kv8_quant16), appends codes and scales, and writes them over row `pos` of its last stage in LDS: the row takes part dequantized.
//   merge     the waves' (m, l, O) in wave order through LDS.  One active chunk: the normalised output.  Several: (O, m, l) into the 132-float
//             workspace records, attn_gqa_combine_kernel (the next launch) adds them in chunk order.  No atomics: same bits run to run.
#include "amq_common.cuh"
#include "amq_kernels.h"
#include "amq_kv8.cuh"

namespace amq {

namespace {

constexpr int KG_D = 128;
constexpr int KG_STAGE_KEYS = 128;
constexpr int KG_TILE = KG_STAGE_KEYS * KG_D;           // 16 KiB of K or of V codes per stage
constexpr int KG_BUF = 2 * KG_TILE + 2 * KG_STAGE_KEYS * 4;     // K | V | K scales | V scales
constexpr int KG_HEAD = 512;                            // in front of the stage buffers: rotated new key [128], new value [128] (fp16)
constexpr int KG_WS_STRIDE = 132;                       // floats per (query head, chunk) in the workspace: O[128], m, l, pad
constexpr int KG_OM_STRIDE = 132;                       // floats per (wave, query row) of the cross-wave merge area
constexpr size_t KG_LDS = KG_HEAD + 2 * (size_t)KG_BUF;
static_assert((size_t)(4 * 16 * KG_OM_STRIDE + 4 * 16 * 2) * sizeof(float) <= 2 * (size_t)KG_BUF, "merge area inside the stage buffers");

typedef int kg_v2i __attribute__((ext_vector_type(2)));

struct Kv8GqaArgs {
    const void* q; const void* k; const void* v;
    signed char* kc; float* ks; signed char* vc; float* vs;
    void* out;
    const void* state;          // cur mode: the step-state block; else a device int32 position or null
    const void* rope_table;
    float* ws;
    int pos, n_heads, n_kv_heads, max_seq, n_splits, cur_mode;
    float rope_theta;
    int iters;                  // stages per workgroup (chunk = 128 iters)
};

// LDS-DMA as inline assembly (amq_attn_prefill.hip: ap_glds16): sbase wave-uniform, voff the lane's byte offset, lds_dst wave-uniform; lane l's
// 16 (4) bytes land at lds_dst + 16 l (4 l).  M0 is saved and restored.
__device__ __forceinline__ void kg_glds16(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void kg_glds4(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// 8 codes (two dwords, byte e = element e) -> 8 fp16: byte b under 0x64 is 1024 + b; with the sign bit flipped b = c + 128
__device__ __forceinline__ h8 kg_codes_h8(uint32_t w0, uint32_t w1) {
    const h2 off = bcast((_Float16)1152.0f);
    const uint32_t w[2] = {w0, w1};
    h8 f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const h2 lo = as_h2(__builtin_amdgcn_perm(0x64646464u, w[i], 0x04010400u) ^ 0x00800080u) - off;
        const h2 hi = as_h2(__builtin_amdgcn_perm(0x64646464u, w[i], 0x04030402u) ^ 0x00800080u) - off;
        f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
    }
    return f;
}

__global__ __launch_bounds__(256) void attn_decode_kv8_gqa_kernel(Kv8GqaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = lane & 15, o = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int G = a.n_heads / a.n_kv_heads, h0 = kvh * G;
    int pos;
    if (a.cur_mode) pos = *(const int*)((const char*)a.state + 256);
    else if (a.state) pos = *(const int*)a.state;
    else pos = a.pos;
    if (pos < 0 || pos >= a.max_seq) {              // a position outside the cache: nothing is appended or written, the error word is raised
        if (a.cur_mode && tid == 0 && z == 0 && kvh == 0 && b == 0) *(int*)((char*)const_cast<void*>(a.state) + 260) = 1;
        return;
    }
    const int chunk = KG_STAGE_KEYS * a.iters;
    const int T = pos + 1;
    const int n_act = (T + chunk - 1) / chunk;      // chunks that hold keys: the others leave at once
    if (z >= n_act) return;
    const int t0 = z * chunk;
    const int t1 = t0 + chunk < T ? t0 + chunk : T; // this workgroup's keys: t0 .. t1 - 1
    const int n_it = (t1 - t0 + KG_STAGE_KEYS - 1) / KG_STAGE_KEYS;
    const bool has_new = t1 == T;                   // the chunk that ends at the new token: the one workgroup of this (sequence, kv head) that appends
    const unsigned last_old = pos > 0 ? pos - 1 : 0;    // rows >= pos are never taken from the cache
    const size_t cbase = ((size_t)b * a.n_kv_heads + kvh) * (size_t)a.max_seq;
    const signed char* const kc = a.kc + cbase * KG_D;
    const signed char* const vc = a.vc + cbase * KG_D;
    const float* const ksg = a.ks + cbase;
    const float* const vsg = a.vs + cbase;

    // ---- staging: 9 LDS-DMA instructions per wave and stage
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + KG_HEAD;
    const unsigned rit = 8 * wave + (lane >> 3);                            // row of piece `wave` (piece w + 4 j: + 32 j)
    const unsigned swz = ((lane & 7) ^ ((rit >> 1) & 7)) << 4;              // (row >> 1) & 7 does not depend on j
    auto load_stage = [&](int it) {
        const unsigned dst = lds0 + (it & 1) * KG_BUF;
        const unsigned key0 = (unsigned)(t0 + KG_STAGE_KEYS * it);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned key = key0 + rit + 32 * j;
            key = key < last_old ? key : last_old;
            kg_glds16(kc, key * 128u + swz, dst + (wave + 4 * j) * 1024);
            kg_glds16(vc, key * 128u + swz, dst + KG_TILE + (wave + 4 * j) * 1024);
        }
        unsigned key = key0 + 64 * (wave & 1) + lane;                       // waves 0, 1: the K scales; 2, 3: the V scales
        key = key < last_old ? key : last_old;
        kg_glds4(wave < 2 ? ksg : vsg, key * 4u, dst + 2 * KG_TILE + wave * 256);
    };
    load_stage(0);

    // ---- behind it: the lane's raw query fragments (row r = query head h0 + r; rows past the group repeat its last head: computed, never stored),
    // the cos / sin pairs they rotate with, and -- the first 64 threads of the appending workgroup -- the new key / value
    const int rq = r < G ? r : G - 1;
    const _Float16* const qb = (const _Float16*)a.q + ((size_t)b * a.n_heads + h0 + rq) * KG_D + 16 * o;
    h8 qf[4];                                       // step t: dims 64 (t >> 1) + 16 o + 8 (t & 1) .. + 7
#pragma unroll
    for (int t = 0; t < 4; ++t) qf[t] = *(const h8*)(qb + 64 * (t >> 1) + 8 * (t & 1));
    const h2* const cs_src = a.cur_mode ? (const h2*)a.state : (a.rope_table ? (const h2*)a.rope_table + (size_t)pos * 64 : nullptr);
    h8 cs[2][2];                                    // [t][half]: (cos, sin) of pairs 16 o + 8 t .. + 3 and .. + 4 .. + 7
    _Float16 k0 = 0, k1 = 0, v0 = 0, v1 = 0;
    h2 csk = {(_Float16)1.f, (_Float16)0.f};
    const bool new_lane = has_new && tid < 64;
    if (cs_src) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            cs[t][0] = *(const h8*)(cs_src + 16 * o + 8 * t);
            cs[t][1] = *(const h8*)(cs_src + 16 * o + 8 * t + 4);
        }
        if (new_lane) csk = cs_src[tid];
    } else {                                        // no table, no step state: the pairs from rope_theta (attn_decode_kernel's rope_cs)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i = 16 * o + 8 * t + e;
                float sn, c_;
                sincosf((float)pos * (1.0f / powf(a.rope_theta, (float)(2 * i) / (float)KG_D)), &sn, &c_);
                cs[t][e >> 2][2 * (e & 3)] = (_Float16)c_;
                cs[t][e >> 2][2 * (e & 3) + 1] = (_Float16)sn;
            }
        if (new_lane) {
            float sn, c_;
            sincosf((float)pos * (1.0f / powf(a.rope_theta, (float)(2 * tid) / (float)KG_D)), &sn, &c_);
            csk = (h2){(_Float16)c_, (_Float16)sn};
        }
    }
    if (new_lane) {
        const _Float16* const kn = (const _Float16*)a.k + ((size_t)b * a.n_kv_heads + kvh) * KG_D;
        const _Float16* const vn = (const _Float16*)a.v + ((size_t)b * a.n_kv_heads + kvh) * KG_D;
        k0 = kn[tid]; k1 = kn[tid + 64];
        v0 = vn[tid]; v1 = vn[tid + 64];
    }
    AMQ_WAIT_VM("attn.kv8gqa.landed", 0, "");       // this wave's share of stage 0 and its loads
    // rotation: q' = q * cos + rotate_half(q) * sin in fp16 (HF apply_rotary_pos_emb; the decode kernels' expression): pair (d, d + 64) = fragments t, t + 2
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const h8 lo = qf[t], hi = qf[t + 2];
        h8 nlo, nhi;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const _Float16 c16 = cs[t][e >> 2][2 * (e & 3)], s16 = cs[t][e >> 2][2 * (e & 3) + 1];
            nlo[e] = lo[e] * c16 + (-hi[e]) * s16;
            nhi[e] = hi[e] * c16 + lo[e] * s16;
        }
        qf[t] = nlo; qf[t + 2] = nhi;
    }
    _Float16* const rk = (_Float16*)smem;           // [128] rotated new key | [128] new value
    _Float16* const rv = rk + KG_D;
    if (new_lane) {
        rk[tid] = k0 * csk.x + (-k1) * csk.y; rk[tid + 64] = k1 * csk.x + k0 * csk.y;
        rv[tid] = v0; rv[tid + 64] = v1;
    }
    __syncthreads();                                // every wave's share of stage 0 has landed; rk / rv are visible
    u4 newc = {0u, 0u, 0u, 0u};                     // threads 0 .. 7: the new key's codes of dims 16 tid .. + 15; 8 .. 15: the new value's
    float news = 0.f;
    if (has_new && tid < 16) {
        const bool is_v = tid >> 3;
        const int l8 = tid & 7;
        const _Float16* const src = (is_v ? rv : rk) + 16 * l8;
        newc = kv8_quant16(*(const h8*)src, *(const h8*)(src + 8), &news);
        *(u4*)((is_v ? a.vc : a.kc) + (cbase + (size_t)pos) * KG_D + 16 * l8) = newc;
        if (l8 == 0) (is_v ? a.vs : a.ks)[cbase + (size_t)pos] = news;
    }
    unsigned char* const bufs = smem + KG_HEAD;

    // ---- the stages
    const float scale = 0.08838834764831845f;       // RN32(1 / sqrt 128) = 0x3DB504F3
    f4 oacc[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) oacc[d] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    for (int it = 0; it < n_it; ++it) {
        if (it + 1 < n_it) load_stage(it + 1);      // (its buffer was last read in stage it - 1, behind that stage's barrier)
        unsigned char* const sb = bufs + (it & 1) * KG_BUF;
        float* const kss = (float*)(sb + 2 * KG_TILE);
        float* const vss = kss + KG_STAGE_KEYS;
        if (has_new && it == n_it - 1) {            // the new token's row over the (clamped) row `pos` of the stage: codes where the swizzle puts them
            const int lr = pos - (t0 + KG_STAGE_KEYS * it);
            if (tid < 16) {
                const int l8 = tid & 7;
                *(u4*)(sb + (tid >> 3) * KG_TILE + lr * KG_D + ((l8 ^ ((lr >> 1) & 7)) << 4)) = newc;
                if (l8 == 0) ((tid >> 3) ? vss : kss)[lr] = news;
            }
            __syncthreads();
        }
        const int kw = t0 + KG_STAGE_KEYS * it + 32 * wave;       // this wave's first key of the stage
        if (kw < t1) {
            f4 st[2];
#pragma unroll
            for (int kl = 0; kl < 2; ++kl) {
                const int row = 32 * wave + 16 * kl + r, sw = (row >> 1) & 7;
                const u4 ka = *(const u4*)(sb + row * KG_D + ((o ^ sw) << 4));
                const u4 kb = *(const u4*)(sb + row * KG_D + (((o + 4) ^ sw) << 4));
                st[kl] = (f4){0.f, 0.f, 0.f, 0.f};
                st[kl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kg_codes_h8(ka.x, ka.y), qf[0], st[kl], 0, 0, 0);
                st[kl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kg_codes_h8(ka.z, ka.w), qf[1], st[kl], 0, 0, 0);
                st[kl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kg_codes_h8(kb.x, kb.y), qf[2], st[kl], 0, 0, 0);
                st[kl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kg_codes_h8(kb.z, kb.w), qf[3], st[kl], 0, 0, 0);
            }
            float sv[8], vsc[8];
            float mt = -INFINITY, S = 0.f;
#pragma unroll
            for (int kl = 0; kl < 2; ++kl) {
                const f4 ksv = *(const f4*)(kss + 32 * wave + 16 * kl + 4 * o);
                const f4 vsv = *(const f4*)(vss + 32 * wave + 16 * kl + 4 * o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool live = (kw + 16 * kl + 4 * o + i) < t1;
                    sv[4 * kl + i] = live ? (st[kl][i] * ksv[i]) * scale : -INFINITY;
                    vsc[4 * kl + i] = live ? vsv[i] : 0.f;
                    mt = fmaxf(mt, sv[4 * kl + i]);
                    S = fmaxf(S, vsc[4 * kl + i]);
                }
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));     // the wave's first key is inside the chunk: finite
            S = fmaxf(S, __shfl_xor(S, 16));
            S = fmaxf(S, __shfl_xor(S, 32));        // the largest V scale of the wave's 32 keys
            const float rS = S > 0.f ? 1.0f / S : 0.f;
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __expf(m_run - m_new);      // e^(-inf) = 0 on the wave's first stage
            m_run = m_new;
            h8 pb;
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float p = __expf(sv[e] - m_new);
                ls += p;
                pb[e] = (_Float16)(p * (vsc[e] * rS));
            }
            l_run = l_run * alpha + ls;
            // the 16-lane group's 8 rows x 16 bytes: lane j -> row (16 (j >> 3) + 4 o + ((j >> 1) & 3)) of the wave's 32, bytes 8 (j & 1) .. + 7 of the chunk
            const int vrow = 32 * wave + 16 * (r >> 3) + 4 * o + ((r >> 1) & 3), vsw = (vrow >> 1) & 7;
            const unsigned char* const vrp = sb + KG_TILE + vrow * KG_D + 8 * (r & 1);
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const kg_v2i c = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) kg_v2i*)(vrp + ((d ^ vsw) << 4)));
                const f4 tv = __builtin_amdgcn_mfma_f32_16x16x32_f16(kg_codes_h8((uint32_t)c.x, (uint32_t)c.y), pb, (f4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) oacc[d][i] = __builtin_fmaf(S, tv[i], oacc[d][i] * alpha);
            }
        }
        AMQ_WAIT_VM("attn.kv8gqa.stage", 0, "");    // this wave's share of the next stage
        __syncthreads();                            // ... every wave's; and this stage's buffer has been read
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    // ---- merge the waves' (m, l, O) in wave order (the stage buffers are free: the loop ends on a barrier): lane holds O^T[d = 16 db + 4 o + i][query r]
    float* const Om = (float*)bufs;                 // [4][16][KG_OM_STRIDE]
    float* const mlw = Om + 4 * 16 * KG_OM_STRIDE;  // [4][16][2]
#pragma unroll
    for (int d = 0; d < 8; ++d) *(f4*)(Om + ((size_t)wave * 16 + r) * KG_OM_STRIDE + 16 * d + 4 * o) = oacc[d];
    if (o == 0) { mlw[(wave * 16 + r) * 2] = m_run; mlw[(wave * 16 + r) * 2 + 1] = l_run; }
    __syncthreads();
    const bool single = n_act == 1;                 // wave-uniform
    for (int idx = tid; idx < G * KG_D; idx += 256) {
        const int qh = idx >> 7, d = idx & 127;
        float M = mlw[qh * 2];
#pragma unroll
        for (int w = 1; w < 4; ++w) M = fmaxf(M, mlw[(w * 16 + qh) * 2]);
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = __expf(mlw[(w * 16 + qh) * 2] - M);       // a wave that never had keys: e^(-inf) = 0
            L += mlw[(w * 16 + qh) * 2 + 1] * f;
            O += Om[((size_t)w * 16 + qh) * KG_OM_STRIDE + d] * f;
        }
        if (single) {
            ((_Float16*)a.out)[((size_t)b * a.n_heads + h0 + qh) * KG_D + d] = (_Float16)(O / L);
        } else {
            float* const wz = a.ws + (((size_t)b * a.n_heads + h0 + qh) * (size_t)a.n_splits + z) * KG_WS_STRIDE;
            wz[d] = O;                              // (read by attn_gqa_combine_kernel, the next launch)
            if (d == 0) { wz[KG_D] = M; wz[KG_D + 1] = L; }
        }
    }
}

}  // namespace

// stages of 128 keys per workgroup for a cache of max_seq rows cut n_splits ways
int attn_decode_kv8_gqa_iters(int max_seq, int n_splits) {
    const int per = (max_seq + n_splits - 1) / n_splits;
    return (per + KG_STAGE_KEYS - 1) / KG_STAGE_KEYS;
}

hipError_t launch_attn_decode_kv8_gqa(const Kv8Args& a, int batch, int n_splits, void* ws, hipStream_t st) {
    StreamDevice sd_(st);
    const bool cur = a.step_state != nullptr;
    const int iters = attn_decode_kv8_gqa_iters(a.max_seq, n_splits);
    Kv8GqaArgs g{a.q, a.k, a.v, (signed char*)a.kc8, (float*)a.ks, (signed char*)a.vc8, (float*)a.vs, a.out,
                 cur ? a.step_state : (const void*)a.pos_dev, cur ? nullptr : a.rope_table, (float*)ws, a.pos, a.n_heads, a.n_kv_heads, a.max_seq,
                 n_splits, (int)cur, a.rope_theta, iters};
    static unsigned long long attr_done = 0;
    if (hipError_t e = ensure_dyn_lds(attr_done, (const void*)attn_decode_kv8_gqa_kernel, (int)KG_LDS)) return e;
    hipLaunchKernelGGL(attn_decode_kv8_gqa_kernel, dim3(a.n_kv_heads, batch, n_splits), dim3(256), KG_LDS, st, g);
    if (hipError_t e = hipGetLastError()) return e;
    if (n_splits == 1) return hipSuccess;           // one chunk: the kernel has written the output itself
    return launch_attn_gqa_combine(ws, a.out, g.state, a.pos, (int)cur, a.n_heads, batch, a.max_seq, n_splits, KG_STAGE_KEYS * iters, st);
}

}  // namespace amq
