// amq_attn_kv8_i8.hip -- decode step over the 8-bit KV cache on the INTEGER matrix cores, gfx950: v_mfma_i32_16x16x64_i8.
//
// The cache's int8 rows are matrix operands exactly as they lie in memory: no instruction turns a code into anything (amq_attn_kv8_gqa.hip
// spends 1.5 VALU operations a code on fp16), so nothing is gained by sharing a conversion across a head group and the G = n_heads /
// n_kv_heads = 1 .. 16 query heads of a kv head (multi-head models included) are the rows of one 16-row block; rows past G repeat the last
// head and are never stored.  q and the probability weights are int8 too, in TWO planes each (one plane: 1e-2 .. 7e-2 of max |out|).
// Grid (kv head, sequence, chunk), 128 threads = 2 waves; a chunk is `iters` stages of 128 keys, wave w owns keys 64 w .. 64 w + 63 of a stage.
//
//   maps      (probed on the device with one-hot integer operands)  A and B of v_mfma_i32_16x16x64_i8: lane (r = lane & 15, o = lane >> 4)
//             holds 16 bytes of row (column) r; byte e of lane group o of A meets byte e of lane group o of B -- WHICH k index that is never
//             matters here, both operands are always laid out by one map.  D: lane (c, o), register i = D[4 o + i][c].  ds_read_b64_tr_b8:
//             the 16 lanes of a group address 8 rows x 16 bytes (lane j: row j >> 1, bytes 8 (j & 1) .. + 7); lane r receives byte r of the
//             8 rows, row j >> 1 in byte j >> 1.
//   staging   as amq_attn_kv8_gqa.hip: a stage = the RAW rows, 128 x 128 B of K codes, of V codes, 2 x 128 fp32 scales (33 KiB) by LDS-DMA into
//             one of two buffers, stage it + 1 in flight under stage it.  A DMA instruction moves 8 rows (lane l: row l >> 3, 16-byte chunk
//             l & 7); wave w moves pieces w, w + 2, .. w + 14 of K and of V, the K scales of keys 64 w .. + 63 and the V scales of the same
//             (18 instructions a wave and stage).  LDS position p of row x holds chunk p ^ ((x >> 1) & 7): 16 rows x one chunk cover all 64
//             banks once, for ds_read_b128 and for the transposing reads.  Rows at or past the position are clamped to the last cached row.
//   query     rotated with the fp16 expression of every decode kernel, in registers: lane (r, o) holds dims 16 o .. + 15 and 64 + 16 o .. + 15 of
//             head r -- the rotation's pairs, and the B operand's bytes of the two instructions that cover 128 dims.  a = max |q_i| (the lane's
//             32, then the 4 lane groups), sq = a / 127, x = q / sq, qh = clamp(rint x), ql = clamp(rint((x - qh) 254)); a == 0: zero planes.
//   scores    S^T = K . Q^T per 16-key tile: A = ds_read_b128 of chunk o (o + 4) of key row r, straight into the operand; 2 instructions a plane.
//             D = 254 Dh + Dl exact in int32 (|D| <= 254 * 128 * 127^2 < 2^31; v_mad_i32_i24: |Dh| < 2^23);
//             s = float(D) (sq / 254) ks RN32(1 / sqrt 128) in fp32.  Four tiles give lane (head c, o) keys 16 kl + 4 o + i of the wave's 64.
//   softmax   online, fp32, per wave and head: running maximum m, sum l of the UNQUANTIZED p, accumulators rescaled by e^(m_old - m_new).
//   P.V       O^T = V^T . W^T per 64 keys.  w = p vs in fp32 (the V scale never enters anything narrower), S = the block's largest w of the head,
//             y = w (127 / S), wh = rint y (0 .. 127), wl = clamp(rint((y - wh) 254)).  B byte e = 4 kl + i = the key 16 kl + 4 o + i the score
//             registers hold; A = two ds_read_b64_tr_b8 of the row-major tile whose 16 lanes address exactly those rows (lane j: key
//             16 (j >> 3) + 4 o + ((j >> 1) & 3), then + 32).  T = 254 Th + Tl exact in int32, O <- alpha O + (S / (127 * 254)) float(T).
//             A masked key has w = 0; S == 0 contributes nothing.
//   new row   the workgroup whose chunk ends at the new token quantizes k / v (kv8_quant16), appends codes and scales, and writes them over row
//             `pos` of its last stage in LDS: the row takes part dequantized; the cache is bit for bit the per-head launch's.
//   merge     the two waves' (m, l, O) in wave order through LDS.  One active chunk: the normalised output.  Several: (O, m, l) into the 132-float
//             workspace records, attn_gqa_combine_kernel (the next launch) adds them in chunk order.  No atomics: same bits run to run.
#include "amq_common.cuh"
#include "amq_kernels.h"
#include "amq_kv8.cuh"

namespace amq {

namespace {

constexpr int KI_D = 128;
constexpr int KI_STAGE_KEYS = 128;
constexpr int KI_WAVES = 2;
constexpr int KI_TILE = KI_STAGE_KEYS * KI_D;           // 16 KiB of K or of V codes per stage
constexpr int KI_BUF = 2 * KI_TILE + 2 * KI_STAGE_KEYS * 4;     // K | V | K scales | V scales
constexpr int KI_HEAD = 512;                            // in front of the stage buffers: rotated new key [128], new value [128] (fp16)
constexpr int KI_WS_STRIDE = 132;                       // floats per (query head, chunk) in the workspace: O[128], m, l, pad
constexpr int KI_OM_STRIDE = 132;                       // floats per (wave, query row) of the cross-wave merge area
constexpr size_t KI_LDS = KI_HEAD + 2 * (size_t)KI_BUF;
static_assert((size_t)(KI_WAVES * 16 * KI_OM_STRIDE + KI_WAVES * 16 * 2) * sizeof(float) <= 2 * (size_t)KI_BUF, "merge area inside the stage buffers");

typedef int ki_v2i __attribute__((ext_vector_type(2)));
typedef int ki_v4i __attribute__((ext_vector_type(4)));

struct Kv8I8Args {
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

// LDS-DMA as inline assembly (amq_attn_kv8_gqa.hip: kg_glds16 / kg_glds4): sbase wave-uniform, voff the lane's byte offset, lds_dst
// wave-uniform; lane l's 16 (4) bytes land at lds_dst + 16 l (4 l).  M0 is saved and restored.
__device__ __forceinline__ void ki_glds16(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void ki_glds4(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

__device__ __forceinline__ float ki_max16(float v) {       // over the 4 lanes that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ uint32_t ki_pack4(const int* c) {
    return ((uint32_t)c[0] & 0xFFu) | (((uint32_t)c[1] & 0xFFu) << 8) | (((uint32_t)c[2] & 0xFFu) << 16) | ((uint32_t)c[3] << 24);
}
// y >= 0 or signed, |high plane| <= 127: the two int8 planes whose 254 hi + lo is y to 1 / 508
__device__ __forceinline__ void ki_planes(float y, int* hi, int* lo) {
    const float h = fminf(fmaxf(rintf(y), -127.f), 127.f);
    const float l = fminf(fmaxf(rintf((y - h) * 254.f), -127.f), 127.f);
    *hi = (int)h; *lo = (int)l;
}
__device__ __forceinline__ ki_v4i ki_mfma(ki_v4i a, ki_v4i b, ki_v4i c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(64 * KI_WAVES) void attn_decode_kv8_i8_kernel(Kv8I8Args a) {
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
    const int chunk = KI_STAGE_KEYS * a.iters;
    const int T = pos + 1;
    const int n_act = (T + chunk - 1) / chunk;      // chunks that hold keys: the others leave at once
    if (z >= n_act) return;
    const int t0 = z * chunk;
    const int t1 = t0 + chunk < T ? t0 + chunk : T; // this workgroup's keys: t0 .. t1 - 1
    const int n_it = (t1 - t0 + KI_STAGE_KEYS - 1) / KI_STAGE_KEYS;
    const bool has_new = t1 == T;                   // the chunk that ends at the new token: the one workgroup of this (sequence, kv head) that appends
    const unsigned last_old = pos > 0 ? pos - 1 : 0;    // rows >= pos are never taken from the cache
    const size_t cbase = ((size_t)b * a.n_kv_heads + kvh) * (size_t)a.max_seq;
    const signed char* const kc = a.kc + cbase * KI_D;
    const signed char* const vc = a.vc + cbase * KI_D;
    const float* const ksg = a.ks + cbase;
    const float* const vsg = a.vs + cbase;

    // ---- staging: 18 LDS-DMA instructions per wave and stage
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + KI_HEAD;
    const unsigned rit = 8 * wave + (lane >> 3);                            // row of piece `wave` (piece w + 2 j: + 16 j)
    const unsigned swz = ((lane & 7) ^ ((rit >> 1) & 7)) << 4;              // (row >> 1) & 7 does not depend on j
    auto load_stage = [&](int it) {
        const unsigned dst = lds0 + (it & 1) * KI_BUF;
        const unsigned key0 = (unsigned)(t0 + KI_STAGE_KEYS * it);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned key = key0 + rit + 16 * j;
            key = key < last_old ? key : last_old;
            ki_glds16(kc, key * 128u + swz, dst + (wave + 2 * j) * 1024);
            ki_glds16(vc, key * 128u + swz, dst + KI_TILE + (wave + 2 * j) * 1024);
        }
        unsigned key = key0 + 64 * wave + lane;
        key = key < last_old ? key : last_old;
        ki_glds4(ksg, key * 4u, dst + 2 * KI_TILE + wave * 256);
        ki_glds4(vsg, key * 4u, dst + 2 * KI_TILE + KI_STAGE_KEYS * 4 + wave * 256);
    };
    load_stage(0);

    // ---- behind it: the lane's raw query fragments (row r = query head h0 + r; rows past the group repeat its last head: computed, never stored),
    // the cos / sin pairs they rotate with, and -- the first 64 threads of the appending workgroup -- the new key / value
    const int rq = r < G ? r : G - 1;
    const _Float16* const qb = (const _Float16*)a.q + ((size_t)b * a.n_heads + h0 + rq) * KI_D + 16 * o;
    h8 qf[4];                                       // fragment t: dims 64 (t >> 1) + 16 o + 8 (t & 1) .. + 7
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
                sincosf((float)pos * (1.0f / powf(a.rope_theta, (float)(2 * i) / (float)KI_D)), &sn, &c_);
                cs[t][e >> 2][2 * (e & 3)] = (_Float16)c_;
                cs[t][e >> 2][2 * (e & 3) + 1] = (_Float16)sn;
            }
        if (new_lane) {
            float sn, c_;
            sincosf((float)pos * (1.0f / powf(a.rope_theta, (float)(2 * tid) / (float)KI_D)), &sn, &c_);
            csk = (h2){(_Float16)c_, (_Float16)sn};
        }
    }
    if (new_lane) {
        const _Float16* const kn = (const _Float16*)a.k + ((size_t)b * a.n_kv_heads + kvh) * KI_D;
        const _Float16* const vn = (const _Float16*)a.v + ((size_t)b * a.n_kv_heads + kvh) * KI_D;
        k0 = kn[tid]; k1 = kn[tid + 64];
        v0 = vn[tid]; v1 = vn[tid + 64];
    }
    AMQ_WAIT_VM("attn.kv8i8.landed", 0, "");        // this wave's share of stage 0 and its loads
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
    // the two int8 planes of the head's rotated query: B operand of instruction s = bytes of fragments 2 s, 2 s + 1
    float qa = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) qa = fmaxf(qa, fabsf((float)qf[t][e]));
    qa = ki_max16(qa);
    const float sq = qa / 127.f;
    ki_v4i qh[2], ql[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            int hi4[4], lo4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = qa == 0.f ? 0.f : (float)qf[2 * s + (w >> 1)][4 * (w & 1) + e] / sq;
                ki_planes(x, &hi4[e], &lo4[e]);
            }
            qh[s][w] = (int)ki_pack4(hi4);
            ql[s][w] = (int)ki_pack4(lo4);
        }
    const float sqs = sq / 254.f;

    _Float16* const rk = (_Float16*)smem;           // [128] rotated new key | [128] new value
    _Float16* const rv = rk + KI_D;
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
        *(u4*)((is_v ? a.vc : a.kc) + (cbase + (size_t)pos) * KI_D + 16 * l8) = newc;
        if (l8 == 0) (is_v ? a.vs : a.ks)[cbase + (size_t)pos] = news;
    }
    unsigned char* const bufs = smem + KI_HEAD;

    // ---- the stages
    const float scale = 0.08838834764831845f;       // RN32(1 / sqrt 128) = 0x3DB504F3
    const ki_v4i zero4 = {0, 0, 0, 0};
    f4 oacc[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) oacc[d] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    for (int it = 0; it < n_it; ++it) {
        if (it + 1 < n_it) load_stage(it + 1);      // (its buffer was last read in stage it - 1, behind that stage's barrier)
        unsigned char* const sb = bufs + (it & 1) * KI_BUF;
        float* const kss = (float*)(sb + 2 * KI_TILE);
        float* const vss = kss + KI_STAGE_KEYS;
        if (has_new && it == n_it - 1) {            // the new token's row over the (clamped) row `pos` of the stage: codes where the swizzle puts them
            const int lr = pos - (t0 + KI_STAGE_KEYS * it);
            if (tid < 16) {
                const int l8 = tid & 7;
                *(u4*)(sb + (tid >> 3) * KI_TILE + lr * KI_D + ((l8 ^ ((lr >> 1) & 7)) << 4)) = newc;
                if (l8 == 0) ((tid >> 3) ? vss : kss)[lr] = news;
            }
            __syncthreads();
        }
        const int kw = t0 + KI_STAGE_KEYS * it + 64 * wave;       // this wave's first key of the stage
        if (kw < t1) {
            float sv[16], wv[16];
            float mt = -INFINITY;
#pragma unroll
            for (int kl = 0; kl < 4; ++kl) {
                const int row = 64 * wave + 16 * kl + r, sw = (row >> 1) & 7;
                const ki_v4i ka = *(const ki_v4i*)(sb + row * KI_D + ((o ^ sw) << 4));
                const ki_v4i kb = *(const ki_v4i*)(sb + row * KI_D + (((o + 4) ^ sw) << 4));
                const ki_v4i dh = ki_mfma(kb, qh[1], ki_mfma(ka, qh[0], zero4));
                const ki_v4i dl = ki_mfma(kb, ql[1], ki_mfma(ka, ql[0], zero4));
                const f4 ksv = *(const f4*)(kss + 64 * wave + 16 * kl + 4 * o);
                const f4 vsv = *(const f4*)(vss + 64 * wave + 16 * kl + 4 * o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool live = (kw + 16 * kl + 4 * o + i) < t1;
                    const int D = __mul24(dh[i], 254) + dl[i];
                    sv[4 * kl + i] = live ? (((float)D * sqs) * ksv[i]) * scale : -INFINITY;
                    wv[4 * kl + i] = live ? vsv[i] : 0.f;
                    mt = fmaxf(mt, sv[4 * kl + i]);
                }
            }
            mt = ki_max16(mt);                      // the wave's first key is inside the chunk: finite
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __expf(m_run - m_new);      // e^(-inf) = 0 on the wave's first stage
            m_run = m_new;
            float ls = 0.f, S = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __expf(sv[e] - m_new);
                ls += p;
                wv[e] = p * wv[e];
                S = fmaxf(S, wv[e]);
            }
            l_run = l_run * alpha + ls;
            S = ki_max16(S);                        // the head's largest weight of the wave's 64 keys
            const float rS = S > 0.f ? 127.f / S : 0.f;
            const float So = S * (1.0f / (127.f * 254.f));
            ki_v4i wh, wl;
#pragma unroll
            for (int kl = 0; kl < 4; ++kl) {
                int hi4[4], lo4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) ki_planes(wv[4 * kl + i] * rS, &hi4[i], &lo4[i]);
                wh[kl] = (int)ki_pack4(hi4);
                wl[kl] = (int)ki_pack4(lo4);
            }
            // the 16-lane group's 8 rows x 16 bytes: lane j -> row (16 (j >> 3) + 4 o + ((j >> 1) & 3)) of the wave's 64 (second read: + 32), bytes 8 (j & 1) .. + 7
            const int vrow = 64 * wave + 16 * (r >> 3) + 4 * o + ((r >> 1) & 3), vsw = (vrow >> 1) & 7;
            const unsigned char* const vrp = sb + KI_TILE + vrow * KI_D + 8 * (r & 1);
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const ki_v2i c0 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) ki_v2i*)(vrp + ((d ^ vsw) << 4)));
                const ki_v2i c1 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) ki_v2i*)(vrp + 32 * KI_D + ((d ^ vsw) << 4)));
                const ki_v4i va = {c0.x, c0.y, c1.x, c1.y};
                const ki_v4i th = ki_mfma(va, wh, zero4);
                const ki_v4i tl = ki_mfma(va, wl, zero4);
#pragma unroll
                for (int i = 0; i < 4; ++i) oacc[d][i] = __builtin_fmaf(So, (float)(__mul24(th[i], 254) + tl[i]), oacc[d][i] * alpha);
            }
        }
        AMQ_WAIT_VM("attn.kv8i8.stage", 0, "");     // this wave's share of the next stage
        __syncthreads();                            // ... every wave's; and this stage's buffer has been read
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    // ---- merge the waves' (m, l, O) in wave order (the stage buffers are free: the loop ends on a barrier): lane holds O^T[d = 16 db + 4 o + i][query r]
    float* const Om = (float*)bufs;                 // [2][16][KI_OM_STRIDE]
    float* const mlw = Om + KI_WAVES * 16 * KI_OM_STRIDE;   // [2][16][2]
#pragma unroll
    for (int d = 0; d < 8; ++d) *(f4*)(Om + ((size_t)wave * 16 + r) * KI_OM_STRIDE + 16 * d + 4 * o) = oacc[d];
    if (o == 0) { mlw[(wave * 16 + r) * 2] = m_run; mlw[(wave * 16 + r) * 2 + 1] = l_run; }
    __syncthreads();
    const bool single = n_act == 1;                 // wave-uniform
    for (int idx = tid; idx < G * KI_D; idx += 64 * KI_WAVES) {
        const int qhd = idx >> 7, d = idx & 127;
        const float m0 = mlw[qhd * 2], m1 = mlw[(16 + qhd) * 2];
        const float M = fmaxf(m0, m1);
        const float f0 = __expf(m0 - M), f1 = __expf(m1 - M);     // a wave that never had keys: e^(-inf) = 0
        const float L = mlw[qhd * 2 + 1] * f0 + mlw[(16 + qhd) * 2 + 1] * f1;
        const float O = Om[(size_t)qhd * KI_OM_STRIDE + d] * f0 + Om[((size_t)16 + qhd) * KI_OM_STRIDE + d] * f1;
        if (single) {
            ((_Float16*)a.out)[((size_t)b * a.n_heads + h0 + qhd) * KI_D + d] = (_Float16)(O / L);
        } else {
            float* const wz = a.ws + (((size_t)b * a.n_heads + h0 + qhd) * (size_t)a.n_splits + z) * KI_WS_STRIDE;
            wz[d] = O;                              // (read by attn_gqa_combine_kernel, the next launch)
            if (d == 0) { wz[KI_D] = M; wz[KI_D + 1] = L; }
        }
    }
}

}  // namespace

// chunks are whole 128-key stages, the count amq_attn_kv8_gqa.hip's launch uses (attn_decode_kv8_gqa_iters): the combine launch is the same
hipError_t launch_attn_decode_kv8_i8(const Kv8Args& a, int batch, int n_splits, void* ws, hipStream_t st) {
    StreamDevice sd_(st);
    const bool cur = a.step_state != nullptr;
    const int iters = attn_decode_kv8_gqa_iters(a.max_seq, n_splits);
    Kv8I8Args g{a.q, a.k, a.v, (signed char*)a.kc8, (float*)a.ks, (signed char*)a.vc8, (float*)a.vs, a.out,
                cur ? a.step_state : (const void*)a.pos_dev, cur ? nullptr : a.rope_table, (float*)ws, a.pos, a.n_heads, a.n_kv_heads, a.max_seq,
                n_splits, (int)cur, a.rope_theta, iters};
    static unsigned long long attr_done = 0;
    if (hipError_t e = ensure_dyn_lds(attr_done, (const void*)attn_decode_kv8_i8_kernel, (int)KI_LDS)) return e;
    hipLaunchKernelGGL(attn_decode_kv8_i8_kernel, dim3(a.n_kv_heads, batch, n_splits), dim3(64 * KI_WAVES), KI_LDS, st, g);
    if (hipError_t e = hipGetLastError()) return e;
    if (n_splits == 1) return hipSuccess;           // one chunk: the kernel has written the output itself
    return launch_attn_gqa_combine(ws, a.out, g.state, a.pos, (int)cur, a.n_heads, batch, a.max_seq, n_splits, KI_STAGE_KEYS * iters, st);
}

}  // namespace amq
