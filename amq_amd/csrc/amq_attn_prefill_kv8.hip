// amq_attn_prefill_kv8.hip -- causal attention of a prompt chunk over the 8-bit KV cache, gfx950.
//
// S query rows at positions pos0 .. pos0 + S - 1 of every sequence attend the DEQUANTIZED cache rows 0 .. pos0 + s, their own included (stored by
// amq_kv8_store_f16 before the launch): the decode kernels' rule -- a key reads the same at step p and at step p + 1000.  The grid, the operand
// layouts and the per-lane online softmax are attn_prefill_kernel's (amq_attn_prefill.hip): a 256-thread workgroup is (sequence, query head, block
// of 64 QB query rows), wave w keeps the Q fragments of its QB 16-row blocks in registers, keys are walked from key 0 in tiles of 64 at ABSOLUTE
// multiples of 64, workgroups are dealt XCD-contiguous and heaviest block first, and only the diagonal tiles carry the causal compare.  What is
// this kernel's own is how a tile reaches the matrix cores:
//
//   raw stage   a tile's raw bytes -- 64 x 128 B of K codes, the same of V codes, 2 x 64 fp32 scales (16.5 KiB) -- go global -> LDS by LDS-DMA into
//               one of two buffers, tile t + 1 in flight under tile t's arithmetic.  A DMA instruction moves 8 rows (lane l: row l >> 3, 16-byte
//               chunk l & 7, row-major in LDS); wave w moves pieces w and w + 4 of K and of V; wave 0 the K scales, wave 1 the V scales, 4 bytes a
//               lane (a scale row is not 16-byte aligned).  A tile that reaches past key pos0 + S - 1 clamps its rows to that key.
//   convert     ONCE per workgroup: wave w turns the pieces it moved into fp16 operand rows -- a ds_read_b128 of 16 codes, v_perm_b32 puts a byte
//               under 0x64 (1024 + (c + 128)), a packed subtract of 1152 leaves the exact integer (amq_attn_kv8_gqa.hip: 1.5 VALU a code) -- and
//               writes them where attn_prefill_kernel's staging would have put them: K chunk c of row x at position c ^ (x & 15), V chunk c at
//               2 ((c >> 1) ^ (x & 7)) + (c & 1).  96 VALU per wave and tile; converted in registers by every wave it would be four times that,
//               beside 32 QB MFMAs.  One operand buffer (16 KiB K | 16 KiB V), two barriers a tile: the first behind the raw tile landing and the
//               previous tile's operand reads, the second behind the conversion.
//   scores      S^T = K . Q^T on v_mfma_f32_16x16x32_f16 (ds_read_b128 of K rows); a lane holds S^T[key 16 kb + 4 o + i][its query row].  Each is
//               (raw * ks_t) * RN32(1 / sqrt 128) in fp32 -- the per-key scale BEFORE the running maximum; the lane's 16 K scales (and V scales)
//               of a tile are four 16-byte broadcast reads of the raw buffer.  Masked keys have score and V scale SELECTED away.
//   softmax     online, fp32, per lane = per query row, exp2 domain.
//   P.V         O^T = V^T . P^T, V^T through ds_read_b64_tr_b16.  The weight is fp16(p_t (vs_t / Sv)), Sv the largest V scale among the keys of the
//               tile the ROW sees (per row, not per tile: what a row computes never depends on which rows share its workgroup); the product
//               comes out of the MFMAs on a zero accumulator and O <- alpha O + Sv T in fp32 -- always, no "maximum did not move" skip.
// A query row's bits therefore depend on its q, its position and the cache bytes only: not on pos0, S, QB or the batch.  No atomics, no workspace.
//
// gfx950, ROCm 7.2, -amdgpu-mfma-vgpr-form, QB = 1: 163 VGPRs, no scratch, 66560 bytes of dynamic LDS (two workgroups a CU).
#include <type_traits>
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

namespace {

constexpr int PK_BKV = 64, PK_D = 128;
constexpr int PK_CODES = PK_BKV * PK_D;                     // 8 KiB of K or of V codes per tile
constexpr int PK_RAW = 2 * PK_CODES + 2 * PK_BKV * 4;       // K codes | V codes | K scales | V scales
constexpr int PK_OP = PK_BKV * PK_D * 2;                    // 16 KiB: an fp16 operand tile
constexpr int PK_LDS = 2 * PK_RAW + 2 * PK_OP;              // [raw 0 | raw 1 | K operand | V operand] = 66560 bytes
typedef __fp16 pk_v4h __attribute__((__vector_size__(4 * sizeof(__fp16))));

// LDS-DMA as inline assembly (amq_attn_prefill.hip: ap_glds16): sbase wave-uniform, voff the lane's byte offset, lds_dst wave-uniform; lane l's
// 16 (4) bytes land at lds_dst + 16 l (4 l).  M0 is saved and restored.
__device__ __forceinline__ void pk_glds16(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void pk_glds4(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// 8 codes (two dwords, byte e = element e) -> 8 fp16: byte b under 0x64 is 1024 + b; with the sign bit flipped b = c + 128
__device__ __forceinline__ h8 pk_codes_h8(uint32_t w0, uint32_t w1) {
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

template <int QB>
__global__ __launch_bounds__(256, 2) void attn_prefill_kv8_kernel(AttnPrefillKv8Args a) {
    constexpr int BQ = 64 * QB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = lane & 15, o = lane >> 4;
    // workgroup -> (sequence, head, query block): attn_prefill_kernel's order -- one (sequence, head)'s blocks on ONE XCD, heaviest block first
    const int nqb = (a.S + BQ - 1) / BQ;
    const int total = (int)gridDim.x, L = (int)blockIdx.x;
    const int xcd = L & 7, per = total >> 3, rem = total & 7;
    const int vid = xcd * per + (xcd < rem ? xcd : rem) + (L >> 3);
    const int hb = vid / nqb;
    const int qb = nqb - 1 - (vid - hb * nqb), b = hb / a.n_heads, h = hb - b * a.n_heads;
    const int kvh = h / (a.n_heads / a.n_kv_heads);
    const int q0 = qb * BQ;
    const int n_keys_seq = a.pos0 + a.S;                // rows of this sequence's cache slice that hold keys
    const _Float16* qp = (const _Float16*)a.q + (size_t)b * a.q_bstride + (size_t)h * PK_D;
    const size_t cbase = ((size_t)b * a.n_kv_heads + kvh) * (size_t)a.max_seq;
    const signed char* const kc = (const signed char*)a.kc8 + cbase * PK_D;
    const signed char* const vc = (const signed char*)a.vc8 + cbase * PK_D;
    const float* const ksg = (const float*)a.ks + cbase;
    const float* const vsg = (const float*)a.vs + cbase;

    // the wave's Q fragments (B operand of S^T = K . Q^T): lane (r, o) holds Q[row r][32 t + 8 o .. + 8] of each of its QB row blocks
    int qrow[QB], qpos[QB];
    h8 qf[QB][4];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        qrow[qi] = q0 + 16 * (QB * wave + qi) + r;
        const int qrow_c = qrow[qi] < a.S ? qrow[qi] : a.S - 1;      // rows past S: computed, never stored
#pragma unroll
        for (int t = 0; t < 4; ++t) qf[qi][t] = *(const h8*)(qp + (size_t)qrow_c * a.q_rstride + 32 * t + 8 * o);
        qpos[qi] = a.pos0 + qrow[qi];                   // this lane's query attends keys <= qpos
    }

    // causal: this workgroup needs keys 0 .. pos0 + q0 + BQ - 1
    int last_key = a.pos0 + q0 + BQ - 1;
    if (last_key > n_keys_seq - 1) last_key = n_keys_seq - 1;
    const int n_tiles = last_key / PK_BKV + 1;

    // ---- raw stage: 4 (waves 0, 1: 5) LDS-DMA instructions per wave and tile.  The lane offsets of a whole tile are loop invariants and the tile
    // advances a scalar base; only a tile that reaches past the sequence's last key takes the clamped per-lane path.
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned rrow = 8 * wave + (lane >> 3), cch = lane & 7;       // row of piece `wave` (piece wave + 4: + 32), 16-byte chunk of codes
    const unsigned coff = rrow * PK_D + cch * 16;
    auto load_raw = [&](int kt) {
        const unsigned dst = lds0 + (kt & 1) * PK_RAW;
        const float* const sg = wave == 0 ? ksg : vsg;
        if ((kt + 1) * PK_BKV <= n_keys_seq) {
            const size_t t0 = (size_t)kt * PK_BKV;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pk_glds16(kc + t0 * PK_D, coff + j * 4096, dst + (wave + 4 * j) * 1024);
                pk_glds16(vc + t0 * PK_D, coff + j * 4096, dst + PK_CODES + (wave + 4 * j) * 1024);
            }
            if (wave < 2) pk_glds4(sg + t0, lane * 4u, dst + 2 * PK_CODES + wave * 256);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned key = (unsigned)(kt * PK_BKV) + rrow + 32 * j;
                key = key < (unsigned)n_keys_seq ? key : (unsigned)n_keys_seq - 1;      // clamp: such keys are masked below
                pk_glds16(kc, key * 128u + cch * 16, dst + (wave + 4 * j) * 1024);
                pk_glds16(vc, key * 128u + cch * 16, dst + PK_CODES + (wave + 4 * j) * 1024);
            }
            if (wave < 2) {
                unsigned key = (unsigned)(kt * PK_BKV) + lane;
                key = key < (unsigned)n_keys_seq ? key : (unsigned)n_keys_seq - 1;
                pk_glds4(sg, key * 4u, dst + 2 * PK_CODES + wave * 256);
            }
        }
    };
    // ---- convert: the pieces this wave moved -> fp16 operand rows at attn_prefill_kernel's swizzled positions
    unsigned char* const opk = smem + 2 * PK_RAW;
    unsigned char* const opv = opk + PK_OP;
    auto convert = [&](int kt) {
        const unsigned char* const rb = smem + (kt & 1) * PK_RAW;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = (int)rrow + 32 * j, c = (int)cch;
            const u4 kw = *(const u4*)(rb + row * PK_D + c * 16);
            const u4 vw = *(const u4*)(rb + PK_CODES + row * PK_D + c * 16);
            unsigned char* const kd = opk + row * 256;
            *(h8*)(kd + (((2 * c) ^ (row & 15)) << 4)) = pk_codes_h8(kw.x, kw.y);
            *(h8*)(kd + (((2 * c + 1) ^ (row & 15)) << 4)) = pk_codes_h8(kw.z, kw.w);
            unsigned char* const vd = opv + row * 256 + ((c ^ (row & 7)) << 5);      // chunks 2 c, 2 c + 1: one 32-byte segment
            *(h8*)vd = pk_codes_h8(vw.x, vw.y);
            *(h8*)(vd + 16) = pk_codes_h8(vw.z, vw.w);
        }
    };

    f4 oacc[QB][8];
    float m_run[QB], l_run[QB];                         // running max (row-global), running sum (this lane's keys only)
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        m_run[qi] = -INFINITY; l_run[qi] = 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) oacc[qi][d] = (f4){0.f, 0.f, 0.f, 0.f};
    }

    load_raw(0);
    // the Q fragments must have landed before the loop (attn_prefill_kernel: or the compiler waits for them -- and the DMA behind them -- every tile)
#pragma unroll
    for (int qi = 0; qi < QB; ++qi)
#pragma unroll
        for (int t = 0; t < 4; ++t) asm volatile("" ::"v"(qf[qi][t]));

    // the transpose reads' lane base: row 4 o + tq (+ 32 per 32-key step, + 16 for k-slots j >= 4), its swizzle term and the column part
    const int tq = r >> 2, tp = r & 3;
    const int vlane = (4 * o + tq) * 256 + (((4 * o + tq) & 7) << 5) + ((tp >> 1) << 4) + ((tp & 1) << 3);
    const float scale = 0.08838834764831845f;           // RN32(1 / sqrt 128) = 0x3DB504F3
    const float l2e = 1.4426950408889634f;              // scores are scaled in the natural domain, the exponentials run in the exp2 domain
    // One key tile.  DIAG (the tile reaches past the workgroup's first query row) is compile-time: the compare / select pairs exist only in the one
    // to three last tiles of a workgroup.  A select on `true` is the value itself: a row computes the same in either form.
    auto tile = [&](auto DIAGC, int kt) {
        constexpr bool DIAG = decltype(DIAGC)::value;
        AMQ_WAIT_VM("prefill.kv8.raw", 0, "");          // this wave's share of the raw tile has landed
        __syncthreads();                                // ... every wave's; and the previous tile's operand and scale reads are done
        if (kt + 1 < n_tiles) load_raw(kt + 1);       // in flight under this tile's arithmetic (its buffer held tile kt - 1)
        convert(kt);
        __syncthreads();                                // the operand tiles are whole
        const float* const kss = (const float*)(smem + (kt & 1) * PK_RAW + 2 * PK_CODES);
        const float* const vss = kss + PK_BKV;
        const int k0 = kt * PK_BKV;

        // ---- S^T = K . Q^T for the tile's four 16-key blocks (each K fragment feeds the MFMAs of all QB row blocks)
        f4 st[QB][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) st[qi][kb] = (f4){0.f, 0.f, 0.f, 0.f};
            const int row = 16 * kb + r;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const h8 kf = *(const h8*)(opk + row * 256 + (((4 * t + o) ^ r) << 4));
#pragma unroll
                for (int qi = 0; qi < QB; ++qi) st[qi][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[qi][t], st[qi][kb], 0, 0, 0);
            }
        }
        // ---- scale, mask, running max, p = exp2((s - m) log2 e), weights fp16(p (vs / Sv))
        h8 pb[QB][2];                                    // P^T as the B operand of O^T = V^T . P^T, per 32-key step
        float alpha[QB], sv_max[QB];
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
            const int rel = qpos[qi] - k0 - 4 * o;       // key 16 kb + 4 o + i of the tile is visible iff 16 kb + i <= rel (an inline constant each)
            float mt = -INFINITY, sm = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const f4 ksv = *(const f4*)(kss + 16 * kb + 4 * o);
                const f4 vsv = *(const f4*)(vss + 16 * kb + 4 * o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool live = !DIAG || 16 * kb + i <= rel;
                    const float s = (st[qi][kb][i] * ksv[i]) * scale;
                    st[qi][kb][i] = live ? s : -INFINITY;
                    mt = fmaxf(mt, st[qi][kb][i]);
                    sm = fmaxf(sm, live ? vsv[i] : 0.f);
                }
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            sm = fmaxf(sm, __shfl_xor(sm, 16));
            sm = fmaxf(sm, __shfl_xor(sm, 32));          // the largest V scale among the tile's keys this ROW sees (0: it sees none)
            const float rs = sm > 0.f ? 1.0f / sm : 0.f;
            const float m_new = fmaxf(m_run[qi], mt);    // key 0 is visible to every query: finite from the first tile on
            alpha[qi] = __builtin_amdgcn_exp2f((m_run[qi] - m_new) * l2e);       // exp2(-inf) = 0 on the first tile; exactly 1 if the maximum stayed
            m_run[qi] = m_new;
            sv_max[qi] = sm;
            const float nm = -m_new * l2e;
            float ls = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const f4 vsv = *(const f4*)(vss + 16 * kb + 4 * o);          // (read again: sixteen registers less across the row maximum)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool live = !DIAG || 16 * kb + i <= rel;
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qi][kb][i], l2e, nm));
                    ls += p;                                                  // fp32 softmax denominator
                    pb[qi][kb >> 1][4 * (kb & 1) + i] = (_Float16)(p * ((live ? vsv[i] : 0.f) * rs));
                }
            }
            l_run[qi] = l_run[qi] * alpha[qi] + ls;
        }
        // ---- O^T <- alpha O^T + Sv (V^T . P^T): A operand through the transpose read (attn_prefill_kernel's addressing), zero accumulator
        // (row & 7 = 4 (o & 1) + tq is the same for every row a lane addresses: the swizzle is one xor of the lane's base with d << 5,
        //  the 32-key step and the + 16 rows are immediates)
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            f4 tv[QB];
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) tv[qi] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                // rows 32 ks + 4 o + tq (k-slots j < 4) and + 16 (j >= 4), columns 16 d + 4 tp: 32-byte segment d ^ (row & 7) of the row
                const int off0 = (vlane ^ (d << 5)) + ks * (32 * 256);
                h8 vf;
                const pk_v4h t0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) pk_v4h*)(opv + off0));
                const pk_v4h t1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) pk_v4h*)(opv + off0 + 16 * 256));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    vf[i] = (_Float16)t0[i];
                    vf[4 + i] = (_Float16)t1[i];
                }
#pragma unroll
                for (int qi = 0; qi < QB; ++qi) tv[qi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[qi][ks], tv[qi], 0, 0, 0);
            }
#pragma unroll
            for (int qi = 0; qi < QB; ++qi)
#pragma unroll
                for (int i = 0; i < 4; ++i) oacc[qi][d][i] = __builtin_fmaf(sv_max[qi], tv[qi][i], oacc[qi][d][i] * alpha[qi]);
        }
    };
    // tiles 0 .. n_plain - 1 end at or before the workgroup's first query position: no mask for any row
    int n_plain = (a.pos0 + q0 + 1) / PK_BKV;
    n_plain = n_plain < n_tiles ? n_plain : n_tiles;
    int kt = 0;
    for (; kt < n_plain; ++kt) tile(std::false_type{}, kt);
    for (; kt < n_tiles; ++kt) tile(std::true_type{}, kt);

    // ---- normalise and store: lane holds O[q = qrow][d = 16 db + 4 o + i] (attn_prefill_kernel's two layouts)
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        float l = l_run[qi];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        h4 ov[8];                                       // formed once, ahead of the two layouts: the same bits in both
#pragma unroll
        for (int d = 0; d < 8; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i) ov[d][i] = (_Float16)(oacc[qi][d][i] * inv);
        if (a.out_xfrag) {
            // fragment order (amq_xfrag_f16's layout of the [S, heads * 128] matrix, K tile = head); rows S .. 64 ceil(S / 64) - 1 are zeros
            const int s = qrow[qi];
            if (s < ((a.S + 63) & ~63)) {
                _Float16* const xf = (_Float16*)a.out;
                const size_t grp = ((size_t)(s >> 6) * a.n_heads + h) * 16 + ((s & 63) >> 4) * 4;
                const h4 zero = {0, 0, 0, 0};
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const int ox = 2 * (d & 1) + (o >> 1);
                    *(h4*)(xf + ((grp + (d >> 1)) * 64 + 16 * ox + (s & 15)) * 8 + 4 * (o & 1)) = s < a.S ? ov[d] : zero;
                }
            }
        } else if (qrow[qi] < a.S) {
            _Float16* op = (_Float16*)a.out + (size_t)b * a.o_bstride + (size_t)qrow[qi] * a.o_rstride + (size_t)h * PK_D + 4 * o;
#pragma unroll
            for (int d = 0; d < 8; ++d) *(h4*)(op + 16 * d) = ov[d];
        }
    }
}

}  // namespace

// QB = 1 is the form that is built: at QB = 2 (128-row workgroups, a converted tile serving twice the rows) the diagonal loop spilled eight VGPRs
// to scratch under the two-workgroups-a-CU register bound (ROCm 7.2); the kernel stays written over QB for the day it fits.
hipError_t launch_attn_prefill_kv8(const AttnPrefillKv8Args& a, hipStream_t st) {
    StreamDevice sd_(st);
    static unsigned long long attr_done = 0;
    if (hipError_t e = ensure_dyn_lds(attr_done, (const void*)attn_prefill_kv8_kernel<1>, PK_LDS)) return e;
    const int nwg = ((a.S + 63) / 64) * a.n_heads * a.batch;
    hipLaunchKernelGGL(attn_prefill_kv8_kernel<1>, dim3(nwg), dim3(256), PK_LDS, st, a);
    return hipGetLastError();
}

}  // namespace amq
