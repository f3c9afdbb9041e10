// attention.hip -- fused causal grouped-query attention for MI355X (gfx950): forward, dQ, dK/dV of a training step (a decode step's attention against the KV cache:
// attention_decode.hip).
//
// Reference: LlamaSdpaAttention.forward + the 4-D causal/left-padding mask
// (transformers/src/transformers/models/llama/modeling_llama.py:526-614, 981-1100): key j is visible
// to query i iff j <= i and attention_mask[b, j] != 0; softmax in fp32, P cast to bf16 for P.V.
// Rows without a visible key (left-padding rows) produce zeros (don't-care in the reference).
//
// No S x S tensor ever exists in HBM.  One workgroup = 4 waves = 128 rows of one (batch, head);
// K/V (or Q/dO) tiles of 64 rows are staged in LDS, once plain and once transposed.
// The MFMA orientation is chosen so that the softmax row index sits on the LANE in every product:
//   S^T = K . Q^T           A = K rows from LDS, B = Q rows held in registers   -> acc[key rows][q lanes]
//   O^T = V^T . P^T         A = V^T rows from LDS, B = the S^T accumulator itself (cast to bf16)
// so row max / row sum / rescale are per-lane scalars (one cross-half shuffle each), and the
// accumulator of the first product is the B operand of the second with NO data movement: element
// j of a 32x32x16 B fragment built from accumulator registers 8s..8s+7 is k = 16s + 8(j>>2) + 4h + (j&3)
// (h = lane >> 5), and the transposed LDS tile is read in that same k order (two 8-byte reads).
// The backward kernels reuse the scheme with the roles permuted (lanes = queries for dQ, lanes = keys
// for dK/dV, which loops over the query heads of its KV group, so no atomics anywhere).
//
// DROP (head_dim 64, the register-staged kernels): inverted dropout on the probabilities (GPT-2's attn_dropout), ecgb_attn_fwd_dropout / ecgb_attn_bwd_dropout.
// Element (b, hq, query i, key j) is kept iff mix32(seed, ((b Hq + hq) S + i) S + j) >= p 2^32 -- ecgb_dropout_bf16's rule on a contiguous [B Hq, S, S] tensor --
// evaluated again wherever it is needed, never stored.  Z = kept / (1 - p):
//   forward   o = (P o Z) V: only the bf16 operand of the P.V product is masked (row maximum, row sum and lse are the undropped ones), 1 / (1 - p) rides on the
//             final row scale;
//   backward  delta = rowsum(dO o O) with that O, dP = (dO V^T) o Z, dS = P o (dP - delta) scale, dV = (P o Z)^T dO.
// The hash's argument is linear in the index, so its per-lane part (the row for forward / dQ, the key for dK / dV, and the lane half's 4 h offset inside a tile)
// is formed once per kernel, the tile's part once per tile (uniform), and an element adds a constant: mix32_finish -- two 64-bit multiplies -- per score is what is left.
#include <algorithm>
#include <cstdio>
#include <initializer_list>

#include "attention_common.inc"
#include "dropout_math.hpp"

namespace {

template <int D, bool DMA = false, bool DROP = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs A)
{
    static_assert(!DMA || D == 64, "the LDS-DMA staging is written for 128-byte rows");
    static_assert(!DROP || (D == 64 && !DMA), "dropout on the probabilities: head_dim 64, register-staged");
    // two K / V^T tile buffers: the tile after the one being multiplied is written while the others still compute,
    // one barrier per tile.  Dynamic LDS (4 x 128 D bytes + 4 bytes per key: 36 KB at head_dim 64 and S 1024, 139 KB at 256 / 2048).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kTile = 128 * D;                           // bytes of a 64-row tile, plain or transposed
    auto lds_k2 = [&](int i) { return smem + i * (DMA ? 2 * kTile : kTile); };
    auto lds_vt2 = [&](int i) { return DMA ? smem + i * 2 * kTile + kTile : smem + (2 + i) * kTile; };
    float *lds_maskrow = reinterpret_cast<float *>(smem + (DMA ? 6 : 4) * kTile);        // the batch row's key mask up to this block's last key
    const int wave = DMA ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + 127) / 128, A.Hq / A.Hkv, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + head_in;
    const int q0 = qblk * 128;
    const int qi = q0 + wave * 32 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    bf16x8 qf[D / 16];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    unsigned long long drop_row = 0;                         // DROP: the hash argument of (this lane's row, key 4 h)
    if constexpr (DROP) drop_row = A.drop_seed + (unsigned long long)((((long long)b * A.Hq + hq) * A.S + qi) * A.S + 4 * h) * kMixStep;
    f32x16 accO[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) accO[db][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float sc = A.scale * kLog2e;
    const int k_end = min(A.S, q0 + 128);
    const int wave_qmax = q0 + wave * 32 + 31;
    constexpr int NI = D / 64;                               // staging items per thread: a tile is 16 row groups x D / 8 chunks
    const int item = threadIdx.x & 127;
    const bool first_half = threadIdx.x < 128;
    const unsigned short *src = first_half ? K + rowbase * A.ldk : V + rowbase * A.ldv;
    const long long src_ld = first_half ? A.ldk : A.ldv;
    Stage4 st[NI];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) stage_load<D>(st[i], src, src_ld, k0, A.S, item + 128 * i);
    };
    auto write_tile = [&](int buf, int k0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (first_half) stage_write_plain<D>(lds_k2(buf), st[i], item + 128 * i); else stage_write_transposed(lds_vt2(buf), st[i], item + 128 * i);
        }
    };
    // DMA: a tile is 8 instructions of 1 KiB (8 rows of 128 B) per operand, two of each per wave; per-lane byte offsets inside a tile are
    // constants (whole tiles) or clamped to the last key (the one partial tile a sequence can end with); the tile's base is scalar
    const int last_tile = (k_end - 1) / 64;
    unsigned offK[2], offV[2], offKt[2], offVt[2];
    if constexpr (DMA) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (wave * 2 + i) * 8 + (lane >> 3), slot = lane & 7;
            const int ck = slot ^ ((r >> 1) & 7), cv = slot ^ (((r >> 1) & 1) << 2);
            const int rt = min(r, A.S - 1 - last_tile * 64);                 // tail tile: rows past the last key re-read it (masked: keys >= S)
            offK[i] = (unsigned)(((long long)r * A.ldk + ck * 8) * 2);  offKt[i] = (unsigned)(((long long)rt * A.ldk + ck * 8) * 2);
            offV[i] = (unsigned)(((long long)r * A.ldv + cv * 8) * 2);  offVt[i] = (unsigned)(((long long)rt * A.ldv + cv * 8) * 2);
        }
    }
    auto issue_tile = [&](int t, int buf) {                  // UNCONDITIONAL (the caller clamps t): the waits below stay counted
        const bool tail = (t + 1) * 64 > A.S;
        const unsigned char *kb = reinterpret_cast<const unsigned char *>(K + (rowbase + (long long)t * 64) * A.ldk);
        const unsigned char *vb = reinterpret_cast<const unsigned char *>(V + (rowbase + (long long)t * 64) * A.ldv);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb + (tail ? offKt[i] : offK[i])),
                                             (__attribute__((address_space(3))) void *)(lds_k2(buf) + (wave * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb + (tail ? offVt[i] : offV[i])),
                                             (__attribute__((address_space(3))) void *)(lds_vt2(buf) + (wave * 2 + i) * 1024), 16, 0, 0);
        }
    };
    // key mask: the whole row goes to LDS once (keys >= S read as padded).  Fetched per tile by wave 0 right where it was written, the
    // load's memory latency (~1 700 cycles) sat in front of every tile's barrier: a quarter of the kernel.
    if constexpr (DMA) {
        issue_tile(0, 0);
        issue_tile(min(1, last_tile), 1);
        for (int i = threadIdx.x; i < ((k_end + 63) & ~63); i += 256) lds_maskrow[i] = (i < A.S) ? A.mask[rowbase + i] : 0.f;
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // tile 0 (and Q) landed; tile 1 may still be in flight
        __syncthreads();                                     // (drains: the price of one barrier with full waits, once per workgroup)
    } else {
        load_tile(0);
        for (int i = threadIdx.x; i < ((k_end + 63) & ~63); i += 256) lds_maskrow[i] = (i < A.S) ? A.mask[rowbase + i] : 0.f;
        write_tile(0, 0);
        __syncthreads();
    }
    // DMA: this lane's transposing-read address inside a V image for d block 0 / 1 (first read; the second is 8 keys = 1 KiB further down; the other
    // (kb, s2) row groups go into the instruction's offset field): 16-byte chunk c of key row r lies at c ^ 4 ((r >> 1) & 1)
    unsigned vtr[2] = {0, 0};
    if constexpr (DMA) {
        const int a = lr >> 4, q = (lr & 15) >> 2, p = lr & 3;
        const int key = 4 * h + q;
#pragma unroll
        for (int db = 0; db < 2; ++db)
            vtr[db] = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem + kTile + key * 128 +
                      (((db * 4 + 2 * a + (p >> 1)) ^ (((key >> 1) & 1) << 2)) << 4) + (p & 1) * 8;
    }
#ifdef ECGB_PROFILE
    unsigned long long prof_acc[7] = {};
    long long t_prof = clock64();
#endif
    for (int k0 = 0, it = 0; k0 < k_end; k0 += 64, ++it) {
        const bool more = k0 + 64 < k_end;
        const unsigned vimg = DMA ? (unsigned)((it % 3) * 2 * kTile) : 0u;
        if constexpr (DMA) issue_tile(min(it + 2, last_tile), (it + 2) % 3);      // two tiles ahead, into the buffer tile it - 1 left at the last barrier
        else if (more) load_tile(k0 + 64);   // next tile in flight behind the MFMAs
        APROF(0);
        const unsigned char *lds_k = lds_k2(DMA ? it % 3 : it & 1), *lds_vt = lds_vt2(DMA ? it % 3 : it & 1);
        const float *lds_mask = lds_maskrow + k0;
        if (k0 <= wave_qmax) {
            const bool lds_flag = __any(lds_mask[lane] == 0.f);          // the tile holds a padded / out-of-range key
            // masks only matter on tiles that touch the diagonal of this wave's rows or hold padded keys: two code paths chosen per
            // wave and tile (one `if` around the score loop alone is if-converted by hipcc: every tile then paid the ~130 compare /
            // select instructions of the masked form, a third of the loop's vector instructions)
            // (head_dim 128 / 256: one path with the choice inside -- two copies of the wider loop body cost more registers than a
            // wave has, and the MFMA share of a tile is 2-4 x larger there)
            const bool need_mask = (k0 + 63 > q0 + wave * 32) || lds_flag;
            auto tile = [&](auto mode_tag) {
                constexpr int MODE = decltype(mode_tag)::value;          // 0 = no masks, 1 = masks, 2 = decided here
                float p[2][16];
                float tmax = -INFINITY;
                f32x16 sacc[2];                                     // the two key halves' chains interleaved: an MFMA never
#pragma unroll                                                      // waits for the one issued just before it
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < D / 16; ++ks)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
                        sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain<D>(lds_k, kb * 32 + lr, ks, h), qf[ks], sacc[kb], 0, 0, 0);
                // DMA: the eight V^T fragments of the tile are read now, behind the issue of the S products (the wait inside runs under them)
                bf16x8 vfr[2][2][2];                                // [kb][s2][db]
                if constexpr (DMA) {
                    tr_frags4_wait<0, 16 * 128>(vfr[0], vtr[0] + vimg, vtr[0] + vimg + 1024, vtr[1] + vimg, vtr[1] + vimg + 1024);
                    tr_frags4_wait<32 * 128, 48 * 128>(vfr[1], vtr[0] + vimg, vtr[0] + vimg + 1024, vtr[1] + vimg, vtr[1] + vimg + 1024);
                }
                // max3() below is inline asm: hipcc's hazard recogniser does not look inside it, and a vector instruction that reads an
                // MFMA result needs 19 wait states after a 16-pass MFMA (nothing interlocks: the first version read stale registers now
                // and then -- a slightly different running maximum, a softmax that differed in the last bits from run to run).  The
                // accumulators pass through this statement, so everything after it is ordered behind the wait.
                if constexpr (MODE == 0) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sacc[0]), "+v"(sacc[1]));
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const f32x16 &s = sacc[kb];
                    if (MODE == 1 || (MODE == 2 && need_mask)) {
                        float4 mk4[4];                                           // the lane's 16 keys are 4 runs of 4: four 16-byte reads
                        if constexpr (DMA) {
                            f4v mv[4];
                            const unsigned ma = (unsigned)(size_t)(__attribute__((address_space(3))) float *)const_cast<float *>(lds_mask) + 16 * h;
                            if (kb == 0) lds_rows4_wait<0>(mv, ma); else lds_rows4_wait<128>(mv, ma);
#pragma unroll
                            for (int g4 = 0; g4 < 4; ++g4) mk4[g4] = make_float4(mv[g4][0], mv[g4][1], mv[g4][2], mv[g4][3]);
                        } else {
#pragma unroll
                            for (int g4 = 0; g4 < 4; ++g4) mk4[g4] = *reinterpret_cast<const float4 *>(&lds_mask[kb * 32 + 8 * g4 + 4 * h]);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // key inside the tile
                            const float mkv = (r & 3) == 0 ? mk4[r >> 2].x : (r & 3) == 1 ? mk4[r >> 2].y : (r & 3) == 2 ? mk4[r >> 2].z : mk4[r >> 2].w;
                            const bool vis = (k0 + kl <= qi) & (mkv != 0.f);
                            const float v = vis ? s[r] : -INFINITY;
                            p[kb][r] = v;
                            tmax = fmaxf(tmax, v);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; r += 2) { p[kb][r] = s[r]; p[kb][r + 1] = s[r + 1]; tmax = max3(s[r], s[r + 1], tmax); }
                    }
                }
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * sc;      // p holds raw scores; sc > 0, so the maximum scales with them
                APROF(1);
                const float m_new = fmaxf(m, tmax);
                const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;   // no key visible yet: every p below is exp2(-inf) = 0
                const float alpha = fast_exp2(m - m_safe);                     // m = -inf -> 0 (accumulators are still zero then)
                float lsum = 0.f;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { const float e = fast_exp2(__builtin_fmaf(p[kb][r], sc, -m_safe)); p[kb][r] = e; lsum += e; }
                l = l * alpha + lsum;
                m = m_new;
                if (__any(alpha != 1.f)) {   // once the running maxima have settled the accumulators need no rescale
#pragma unroll
                    for (int db = 0; db < D / 32; ++db)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accO[db][r] *= alpha;
                }
                if constexpr (DROP) {                               // the row sum above is the undropped one; the P.V operand below loses the dropped keys
                    const unsigned long long zt = drop_row + (unsigned long long)k0 * kMixStep;
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (mix32_finish(zt + (unsigned long long)(kb * 32 + (r & 3) + 8 * (r >> 2)) * kMixStep) < A.drop_thr) p[kb][r] = 0.f;
                }
                APROF(2);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const bf16x8 pf = frag_from_acc(&p[kb][8 * s2]);
#pragma unroll
                        for (int db = 0; db < D / 32; ++db)
                            accO[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DMA ? vfr[kb][s2][db & 1] : frag_transposed(lds_vt, db * 32 + lr, kb, s2, h),
                                                                               pf, accO[db], 0, 0, 0);
                    }
                APROF(3);
            };
            if constexpr (D > 64) tile(std::integral_constant<int, 2>{});
            else if (need_mask) tile(std::integral_constant<int, 1>{});
            else tile(std::integral_constant<int, 0>{});
        }
        if constexpr (DMA) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // this wave's pieces of tile it + 1 have landed (tile it + 2's four may still fly)
            APROF(4);
            __builtin_amdgcn_s_barrier();                      // ... and everybody else's; all reads of tile it are done
        } else {
            if (more) write_tile((it + 1) & 1, k0 + 64);   // its last readers passed the barrier that ended the previous trip
            APROF(4);
            __syncthreads();
        }
        APROF(5);
#ifdef ECGB_PROFILE
        prof_acc[6] += 1;
#endif
    }
#ifdef ECGB_PROFILE
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 7; ++k) atomicAdd(&g_attn_prof[(threadIdx.x >> 6) * 8 + k], prof_acc[k]);
#endif
    const float lt = l + __shfl_xor(l, 32, 64);
    float inv = lt > 0.f ? 1.f / lt : 0.f;
    if constexpr (DROP) inv *= A.drop_inv;
    store_accT<D / 32>(accO, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h, inv);
    if (qvalid && h == 0) A.lse[((long long)b * A.Hq + hq) * A.S + qi] = lt > 0.f ? m + log2f(lt) : INFINITY;
}

// =====================================================================================================
// backward, dQ (and delta): 1-D grid of ceil(S/128) x Hq x B workgroups (map_block); lanes = queries
template <int D, bool DROP = false>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AttnArgs A)
{
    static_assert(!DROP || D == 64, "dropout on the probabilities: head_dim 64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 3 x 128 D bytes + 4 bytes per key
    constexpr int kTile = 128 * D;
    unsigned char *lds_k = smem, *lds_v = smem + kTile, *lds_kt = smem + 2 * kTile;
    float *lds_maskrow = reinterpret_cast<float *>(smem + 3 * kTile);        // the batch row's key mask up to this block's last key
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + 127) / 128, A.Hq / A.Hkv, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + head_in;
    const int q0 = qblk * 128;
    const int qi = q0 + wave * 32 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    bf16x8 qf[D / 16], dof[D / 16], of[D / 16];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    load_row_frags<D>(dof, A.d_o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    load_row_frags<D>(of, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += bf2f((unsigned short)dof[ks][j]) * bf2f((unsigned short)of[ks][j]);
    delta += __shfl_xor(delta, 32, 64);
    const long long stat = ((long long)b * A.Hq + hq) * A.S + qi;
    if (qvalid && h == 0) A.delta[stat] = delta;
    const float lse = qvalid ? A.lse[stat] : INFINITY;
    unsigned long long drop_row = 0;                         // DROP: the hash argument of (this lane's row, key 4 h)
    if constexpr (DROP) drop_row = A.drop_seed + (unsigned long long)(stat * A.S + 4 * h) * kMixStep;
    f32x16 accQ[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) accQ[db][r] = 0.f;
    const float sc = A.scale * kLog2e;
    const int k_end = min(A.S, q0 + 128);
    const int wave_qmax = q0 + wave * 32 + 31;
    constexpr int NI = D / 64;
    const int item = threadIdx.x & 127;
    const bool first_half = threadIdx.x < 128;
    const unsigned short *src = first_half ? K + rowbase * A.ldk : V + rowbase * A.ldv;
    const long long src_ld = first_half ? A.ldk : A.ldv;
    Stage4 st[NI];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) stage_load<D>(st[i], src, src_ld, k0, A.S, item + 128 * i);
    };
    load_tile(0);
    for (int i = threadIdx.x; i < ((k_end + 63) & ~63); i += 256) lds_maskrow[i] = (i < A.S) ? A.mask[rowbase + i] : 0.f;   // see attn_fwd_kernel
    for (int k0 = 0; k0 < k_end; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (first_half) { stage_write_plain<D>(lds_k, st[i], item + 128 * i); stage_write_transposed(lds_kt, st[i], item + 128 * i); }
            else stage_write_plain<D>(lds_v, st[i], item + 128 * i);
        }
        if (k0 + 64 < k_end) load_tile(k0 + 64);
        __syncthreads();
        if (k0 > wave_qmax) continue;
        const float *lds_mask = lds_maskrow + k0;
        const bool need_mask = (k0 + 63 > q0 + wave * 32) || __any(lds_mask[lane] == 0.f);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain<D>(lds_k, kb * 32 + lr, ks, h), qf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain<D>(lds_v, kb * 32 + lr, ks, h), dof[ks], dp, 0, 0, 0);
            }
            float ds[16];
            if constexpr (DROP) {                                   // dP = (dO V^T) o Z
                const unsigned long long zt = drop_row + (unsigned long long)k0 * kMixStep;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    dp[r] *= mix32_finish(zt + (unsigned long long)(kb * 32 + (r & 3) + 8 * (r >> 2)) * kMixStep) >= A.drop_thr ? A.drop_inv : 0.f;
            }
            if (need_mask) {
                float4 mk4[4];
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) mk4[g4] = *reinterpret_cast<const float4 *>(&lds_mask[kb * 32 + 8 * g4 + 4 * h]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float mkv = (r & 3) == 0 ? mk4[r >> 2].x : (r & 3) == 1 ? mk4[r >> 2].y : (r & 3) == 2 ? mk4[r >> 2].z : mk4[r >> 2].w;
                    const bool vis = (k0 + kl <= qi) & (mkv != 0.f);
                    const float pr = vis ? fast_exp2(__builtin_fmaf(s[r], sc, -lse)) : 0.f;
                    ds[r] = pr * (dp[r] - delta) * A.scale;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(__builtin_fmaf(s[r], sc, -lse)) * (dp[r] - delta) * A.scale;
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 dsf = frag_from_acc(&ds[8 * s2]);
#pragma unroll
                for (int db = 0; db < D / 32; ++db)
                    accQ[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_transposed(lds_kt, db * 32 + lr, kb, s2, h), dsf, accQ[db], 0, 0, 0);
            }
        }
    }
    store_accT<D / 32>(accQ, A.dq + (long long)hq * D, A.lddq, rowbase + qi, qvalid, h, 1.f);
}

// dQ with LDS-DMA staging (head_dim 64): K and V tiles through a ring of three buffers, two tiles ahead, counted waits (see attn_fwd_kernel<64, true>);
// K is read both ways from one image (row fragments for S, transposing reads for dS . K).  The arithmetic of attn_bwd_dq_kernel<64> except that the softmax scale
// multiplies dQ once at the store instead of every dS element: the same bits for head_dim 64's scale of 1/8 (a power of two commutes with the bf16 rounding of dS).
__global__ __launch_bounds__(256) void attn_bwd_dq_dma_kernel(AttnArgs A)
{
    constexpr int D = 64, kTile = 128 * D;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 3 x (K, V) + 4 bytes per key
    auto lds_k3 = [&](int i) { return smem + i * 2 * kTile; };
    auto lds_v3 = [&](int i) { return smem + i * 2 * kTile + kTile; };
    float *lds_maskrow = reinterpret_cast<float *>(smem + 6 * kTile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + 127) / 128, A.Hq / A.Hkv, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + head_in;
    const int q0 = qblk * 128;
    const int qi = q0 + wave * 32 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    bf16x8 qf[D / 16], dof[D / 16], of[D / 16];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    load_row_frags<D>(dof, A.d_o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    load_row_frags<D>(of, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += bf2f((unsigned short)dof[ks][j]) * bf2f((unsigned short)of[ks][j]);
    delta += __shfl_xor(delta, 32, 64);
    const long long stat = ((long long)b * A.Hq + hq) * A.S + qi;
    if (qvalid && h == 0) A.delta[stat] = delta;
    const float lse = qvalid ? A.lse[stat] : INFINITY;
    f32x16 accQ[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) accQ[db][r] = 0.f;
    const float sc = A.scale * kLog2e;
    const int k_end = min(A.S, q0 + 128);
    const int wave_qmax = q0 + wave * 32 + 31;
    const int last_tile = (k_end - 1) / 64;
    unsigned offK[2], offV[2], offKt[2], offVt[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 8 + (lane >> 3), c = (lane & 7) ^ swz_u(r);
        const int rt = min(r, A.S - 1 - last_tile * 64);                 // tail tile: rows past the last key re-read it (masked: keys >= S)
        offK[i] = (unsigned)(((long long)r * A.ldk + c * 8) * 2);  offKt[i] = (unsigned)(((long long)rt * A.ldk + c * 8) * 2);
        offV[i] = (unsigned)(((long long)r * A.ldv + c * 8) * 2);  offVt[i] = (unsigned)(((long long)rt * A.ldv + c * 8) * 2);
    }
    auto issue_tile = [&](int t, int buf) {                  // UNCONDITIONAL (the caller clamps t): the waits below stay counted
        const bool tail = (t + 1) * 64 > A.S;
        const unsigned char *kb = reinterpret_cast<const unsigned char *>(K + (rowbase + (long long)t * 64) * A.ldk);
        const unsigned char *vb = reinterpret_cast<const unsigned char *>(V + (rowbase + (long long)t * 64) * A.ldv);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb + (tail ? offKt[i] : offK[i])),
                                             (__attribute__((address_space(3))) void *)(lds_k3(buf) + (wave * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb + (tail ? offVt[i] : offV[i])),
                                             (__attribute__((address_space(3))) void *)(lds_v3(buf) + (wave * 2 + i) * 1024), 16, 0, 0);
        }
    };
    issue_tile(0, 0);
    issue_tile(min(1, last_tile), 1);
    for (int i = threadIdx.x; i < ((k_end + 63) & ~63); i += 256) lds_maskrow[i] = (i < A.S) ? A.mask[rowbase + i] : 0.f;   // see attn_fwd_kernel
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __syncthreads();
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    unsigned trA[D / 32], trB[D / 32];                       // this lane's transposing-read offsets inside a K image (first / second read)
#pragma unroll
    for (int db = 0; db < D / 32; ++db) { trA[db] = lds0 + tr_off_u(db, lr, h, 0); trB[db] = lds0 + tr_off_u(db, lr, h, 8); }
    for (int k0 = 0, it = 0; k0 < k_end; k0 += 64, ++it) {
        issue_tile(min(it + 2, last_tile), (it + 2) % 3);
        const int buf = it % 3;
        const unsigned char *lds_k = lds_k3(buf), *lds_v = lds_v3(buf);
        const unsigned kimg = (unsigned)(buf * 2 * kTile);
        if (k0 <= wave_qmax) {
            const float *lds_mask = lds_maskrow + k0;
            const bool need_mask = (k0 + 63 > q0 + wave * 32) || __any(lds_mask[lane] == 0.f);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < D / 16; ++ks) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain_u(lds_k, kb * 32 + lr, ks, h), qf[ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain_u(lds_v, kb * 32 + lr, ks, h), dof[ks], dp, 0, 0, 0);
                }
                bf16x8 ktf[2][2];                            // K^T fragments of this key half [s2][db]: read (and waited for) under the products above
                if (kb == 0) tr_frags4_wait<0, 16 * 128>(ktf, trA[0] + kimg, trB[0] + kimg, trA[1] + kimg, trB[1] + kimg);
                else tr_frags4_wait<32 * 128, 48 * 128>(ktf, trA[0] + kimg, trB[0] + kimg, trA[1] + kimg, trB[1] + kimg);
                float ds[16];
                if (need_mask) {
                    f4v mv[4];
                    const unsigned ma = (unsigned)(size_t)(__attribute__((address_space(3))) float *)const_cast<float *>(lds_mask) + 16 * h;
                    if (kb == 0) lds_rows4_wait<0>(mv, ma); else lds_rows4_wait<128>(mv, ma);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float mkv = mv[r >> 2][r & 3];
                        const bool vis = (k0 + kl <= qi) & (mkv != 0.f);
                        const float pr = vis ? fast_exp2(__builtin_fmaf(s[r], sc, -lse)) : 0.f;
                        ds[r] = pr * (dp[r] - delta);                                // the softmax scale multiplies dQ once, at the store
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(__builtin_fmaf(s[r], sc, -lse)) * (dp[r] - delta);
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 dsf = frag_from_acc(&ds[8 * s2]);
#pragma unroll
                    for (int db = 0; db < D / 32; ++db)
                        accQ[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf[s2][db], dsf, accQ[db], 0, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // this wave's pieces of tile it + 1 have landed (tile it + 2's four may still fly)
        __builtin_amdgcn_s_barrier();                        // ... and everybody else's; all reads of tile it are done
    }
    store_accT<D / 32>(accQ, A.dq + (long long)hq * D, A.lddq, rowbase + qi, qvalid, h, A.scale);
}

// =====================================================================================================
// backward, dK and dV: 1-D grid of ceil(S/128) x Hkv x B workgroups (map_block); lanes = keys; loops over the query heads of the group
// DS > 1 (head_dim 256): the d range of the dK / dV accumulators is split over DS workgroups (blockIdx.x % DS): K, V fragments and
// two full accumulator sets of head_dim 256 do not fit one wave's 512 registers; the S and dP products are recomputed per split.
// WHICH: 0 = dK and dV in one pass (head_dim 64 / 128); 1 = dV only, 2 = dK only -- at head_dim 256 the two gradients are two launches,
// each with full-width accumulators: the dV pass needs S alone (K fragments), the dK pass S and dP (K and V fragments), 1.25 x the MFMA
// work of a single pass instead of the 2.5 x of splitting the d range four ways (DS = 4, the first head_dim-256 version: 3.3 ms per
// layer at Gemma-2B's shape).
template <int D, int DS, int WHICH, bool DROP = false>
__device__ __forceinline__ void attn_bwd_dkv_body(const AttnArgs &A, const int block_x, const int b, const int g, const int hsplit = 0)
{
    static_assert(!DROP || (D == 64 && DS == 1 && WHICH == 0), "dropout on the probabilities: head_dim 64, one pass");
    constexpr bool DO_V = WHICH != 2, DO_K = WHICH != 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 4 x 128 D bytes + 512
    constexpr int kTile = 128 * D;
    unsigned char *lds_q = smem, *lds_do = smem + kTile, *lds_qt = smem + 2 * kTile, *lds_dot = smem + 3 * kTile;
    float *lds_lse = reinterpret_cast<float *>(smem + 4 * kTile), *lds_delta = lds_lse + 64;
    constexpr int NB = D / 32 / DS;                          // 32-wide d blocks this workgroup accumulates
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    const int G = A.Hq / A.Hkv;
    const int kk0 = (block_x / DS) * 128, db0 = (block_x % DS) * NB;
    const int ki = kk0 + wave * 32 + lr;
    const bool kvalid = ki < A.S;
    const long long rowbase = (long long)b * A.S;
    bf16x8 kf[D / 16], vf[D / 16];
    load_row_frags<D>(kf, A.k + (long long)g * D, A.ldk, rowbase + ki, kvalid, h);
    if constexpr (DO_K) load_row_frags<D>(vf, A.v + (long long)g * D, A.ldv, rowbase + ki, kvalid, h);
    const bool kvis = kvalid && A.mask[rowbase + (kvalid ? ki : 0)] != 0.f;
    // DROP: the hash argument of (query 4 h, this lane's key); a query row further is drop_qstep more
    unsigned long long drop_key = 0, drop_qstep = 0;
    if constexpr (DROP) {
        drop_qstep = (unsigned long long)A.S * kMixStep;
        drop_key = A.drop_seed + (unsigned long long)(4ll * h * A.S + ki) * kMixStep;
    }
    f32x16 accK[NB], accV[NB];
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accK[db][r] = 0.f; accV[db][r] = 0.f; }
    const float sc = A.scale * kLog2e;
    const int wave_kmin = kk0 + wave * 32;
    constexpr int NI = D / 64;
    const int item = threadIdx.x & 127;
    const bool first_half = threadIdx.x < 128;            // first half stages Q, second half dO
    const int t_begin = (kk0 / 64) * 64;                   // first query tile that can see this key block
    const int tiles_per_head = (A.S - t_begin + 63) / 64;
    const int heads_here = G / (A.head_splits > 1 ? A.head_splits : 1), head_lo = hsplit * heads_here;   // this workgroup's query heads of the group
    const int n_steps = heads_here * tiles_per_head;
    auto src_of = [&](int step, int &t0, long long &stat) -> const unsigned short * {
        const int hq = g * G + head_lo + step / tiles_per_head;
        t0 = t_begin + (step % tiles_per_head) * 64;
        stat = ((long long)b * A.Hq + hq) * A.S;
        return first_half ? A.q + (long long)hq * D + rowbase * A.ldq : A.d_o + (long long)hq * D + rowbase * A.ldo;
    };
    const long long src_ld = first_half ? A.ldq : A.ldo;
    Stage4 st[NI];
    float lse_n = INFINITY, delta_n = 0.f;      // wave 0: the tile's row statistics; head_dim 64: fetched with the tile, one tile ahead
    auto load_step = [&](int step) {
        int t0; long long stat;
        const unsigned short *src = src_of(step, t0, stat);
#pragma unroll
        for (int i = 0; i < NI; ++i) stage_load<D>(st[i], src, src_ld, t0, A.S, item + 128 * i);
        if (D == 64 && threadIdx.x < 64) {
            const bool v = t0 + (int)threadIdx.x < A.S;
            lse_n = v ? A.lse[stat + t0 + threadIdx.x] : INFINITY;
            delta_n = v ? A.delta[stat + t0 + threadIdx.x] : 0.f;
        }
    };
    load_step(0);
    for (int step = 0; step < n_steps; ++step) {
        int t0; long long stat;
        (void)src_of(step, t0, stat);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (first_half) { stage_write_plain<D>(lds_q, st[i], item + 128 * i); if constexpr (DO_K) stage_write_transposed(lds_qt, st[i], item + 128 * i); }
            else { if constexpr (DO_K) stage_write_plain<D>(lds_do, st[i], item + 128 * i); if constexpr (DO_V) stage_write_transposed(lds_dot, st[i], item + 128 * i); }
        }
        if (threadIdx.x < 64) {
            if (D != 64) {                             // wider heads: measured slower a tile ahead (registers)
                const bool v = t0 + (int)threadIdx.x < A.S;
                lse_n = v ? A.lse[stat + t0 + threadIdx.x] : INFINITY;
                delta_n = v ? A.delta[stat + t0 + threadIdx.x] : 0.f;
            }
            lds_lse[threadIdx.x] = lse_n;
            lds_delta[threadIdx.x] = delta_n;
        }
        if (step + 1 < n_steps) load_step(step + 1);      // next tile in flight behind the MFMAs
        __syncthreads();
        if (t0 + 63 < wave_kmin) continue;        // every query of the tile precedes every key of this wave
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain<D>(lds_q, qb * 32 + lr, ks, h), kf[ks], s, 0, 0, 0);
                if constexpr (DO_K) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain<D>(lds_do, qb * 32 + lr, ks, h), vf[ks], dp, 0, 0, 0);
            }
            float pr[16], ds[16];
            unsigned long long zt = 0;                                       // DROP: (the head's first row + the tile's first query, this lane's key)
            if constexpr (DROP) zt = drop_key + (unsigned long long)(stat + t0) * drop_qstep;
            const bool diag = t0 + qb * 32 < wave_kmin + 32;              // some query of the block may precede some key of the wave
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {                                // the lane's 16 queries are 4 runs of 4: 16-byte reads
                const float4 lse4 = *reinterpret_cast<const float4 *>(&lds_lse[qb * 32 + 8 * g4 + 4 * h]);
                const float4 dl4 = *reinterpret_cast<const float4 *>(&lds_delta[qb * 32 + 8 * g4 + 4 * h]);
                const float lse_t[4] = {lse4.x, lse4.y, lse4.z, lse4.w}, dl_t[4] = {dl4.x, dl4.y, dl4.z, dl4.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = 4 * g4 + t;
                    const int ql = qb * 32 + t + 8 * g4 + 4 * h;             // query inside the tile
                    const bool vis = kvis & (!diag | (ki <= t0 + ql));
                    const float e = vis ? fast_exp2(__builtin_fmaf(s[r], sc, -lse_t[t])) : 0.f;
                    if constexpr (DROP) {                                    // dV takes P o Z, dS the undropped P and dP o Z
                        const float z = mix32_finish(zt + (unsigned long long)(qb * 32 + t + 8 * g4) * drop_qstep) >= A.drop_thr ? A.drop_inv : 0.f;
                        pr[r] = e * z;
                        ds[r] = e * (dp[r] * z - dl_t[t]) * A.scale;
                    } else {
                        pr[r] = e;
                        ds[r] = e * (dp[r] - dl_t[t]) * A.scale;
                    }
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 pf = frag_from_acc(&pr[8 * s2]);
                const bf16x8 dsf = frag_from_acc(&ds[8 * s2]);
#pragma unroll
                for (int db = 0; db < NB; ++db) {
                    if constexpr (DO_V) accV[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_transposed(lds_dot, (db0 + db) * 32 + lr, qb, s2, h), pf, accV[db], 0, 0, 0);
                    if constexpr (DO_K) accK[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_transposed(lds_qt, (db0 + db) * 32 + lr, qb, s2, h), dsf, accK[db], 0, 0, 0);
                }
            }
        }
    }
    if (A.head_splits > 1) {                                 // partial sums over this workgroup's heads: fp32 slabs, reduced in order afterwards
        const long long rows_all = (long long)A.B * A.S, slab = rows_all * A.Hkv * D;
        float *base = A.slab + (long long)hsplit * slab + ((long long)g * rows_all) * D + db0 * 32;
        if constexpr (DO_K) store_accT_f32<NB>(accK, base, D, rowbase + ki, kvalid, h);
        if constexpr (DO_V) store_accT_f32<NB>(accV, base + (long long)A.head_splits * slab, D, rowbase + ki, kvalid, h);
        return;
    }
    if constexpr (DO_K) store_accT<NB>(accK, A.dk + (long long)g * D + db0 * 32, A.lddk, rowbase + ki, kvalid, h, 1.f);
    if constexpr (DO_V) store_accT<NB>(accV, A.dv + (long long)g * D + db0 * 32, A.lddv, rowbase + ki, kvalid, h, 1.f);
}

// dK and dV with LDS-DMA staging (head_dim 64): the Q and dO tiles of a step (one query head, 64 queries) and the tile's row statistics (log-sum-exp,
// delta: 256 bytes each, 4 bytes a lane) go global -> LDS through a ring of three buffers, two steps ahead; every wave issues the same five
// instructions per step (two Q pieces, two dO pieces, one statistics row: waves 0 / 1 bring lse / delta, 2 / 3 a copy nobody reads), so one counted
// wait serves all.  Each tile is read both ways from its one image.  A tile that ends past the sequence re-reads the last row (DMA cannot zero):
// those queries are switched off in the visibility test.  The arithmetic of attn_bwd_dkv_kernel<64, 1, 0> except that the softmax scale multiplies dK once at the
// store: the same bits for head_dim 64's scale of 1/8.
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_dma_kernel(AttnArgs A)
{
    constexpr int D = 64, kTile = 128 * D, kStep = 2 * kTile + 1024;      // Q image, dO image, four statistics rows
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 3 x kStep
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    int blk, head_in, group;
    map_block((int)blockIdx.x, (A.S + 127) / 128, 1, A.B * A.Hkv, false, blk, head_in, group);   // key block 0 sees every query: first
    const int b = group / A.Hkv, g = group % A.Hkv;
    const int G = A.Hq / A.Hkv;
    const int kk0 = blk * 128;
    const int ki = kk0 + wave * 32 + lr;
    const bool kvalid = ki < A.S;
    const long long rowbase = (long long)b * A.S;
    bf16x8 kf[D / 16], vf[D / 16];
    load_row_frags<D>(kf, A.k + (long long)g * D, A.ldk, rowbase + ki, kvalid, h);
    load_row_frags<D>(vf, A.v + (long long)g * D, A.ldv, rowbase + ki, kvalid, h);
    const bool kvis = kvalid && A.mask[rowbase + (kvalid ? ki : 0)] != 0.f;
    // query q sees this lane's key iff the key is real and ki <= q < S: one unsigned compare, (q - vis_lo) < vis_n with vis_lo = ki (S for a padded /
    // out-of-range key: vis_n = 0, never true).  (Causal test, key padding and the clamped rows of a tile past the end were two compares, an or and
    // scalar mask arithmetic per element: 133 of a step's 344 vector instructions.)
    const int vis_lo = kvis ? ki : A.S;
    const unsigned vis_n = (unsigned)(A.S - vis_lo);
    f32x16 accK[D / 32], accV[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accK[db][r] = 0.f; accV[db][r] = 0.f; }
    const float sc = A.scale * kLog2e;
    const int wave_kmin = kk0 + wave * 32;
    const int t_begin = (kk0 / 64) * 64;                   // first query tile that can see this key block
    const int tiles_per_head = (A.S - t_begin + 63) / 64;
    const int n_steps = G * tiles_per_head;
    const int tail_rows = A.S - (t_begin + (tiles_per_head - 1) * 64);    // rows of a head's last tile that exist (1..64)
    unsigned offQ[2], offO[2], offQt[2], offOt[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 8 + (lane >> 3), c = (lane & 7) ^ swz_u(r);
        const int rt = min(r, tail_rows - 1);
        offQ[i] = (unsigned)(((long long)r * A.ldq + c * 8) * 2);  offQt[i] = (unsigned)(((long long)rt * A.ldq + c * 8) * 2);
        offO[i] = (unsigned)(((long long)r * A.ldo + c * 8) * 2);  offOt[i] = (unsigned)(((long long)rt * A.ldo + c * 8) * 2);
    }
    const unsigned offS = (unsigned)lane * 4u, offSt = (unsigned)min(lane, tail_rows - 1) * 4u;
    const float *stat_src = (wave & 1) ? A.delta : A.lse;
    auto issue_step = [&](int step, int buf) {               // UNCONDITIONAL (the caller clamps step): the waits below stay counted
        const int hq = g * G + step / tiles_per_head;
        const int ti = step % tiles_per_head;
        const int t0 = t_begin + ti * 64;
        const bool tail = ti == tiles_per_head - 1 && tail_rows < 64;
        const unsigned char *qb = reinterpret_cast<const unsigned char *>(A.q + (long long)hq * D + (rowbase + t0) * A.ldq);
        const unsigned char *ob = reinterpret_cast<const unsigned char *>(A.d_o + (long long)hq * D + (rowbase + t0) * A.ldo);
        const unsigned char *sb = reinterpret_cast<const unsigned char *>(stat_src + ((long long)b * A.Hq + hq) * A.S + t0);
        unsigned char *dst = smem + buf * kStep;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + (tail ? offQt[i] : offQ[i])),
                                             (__attribute__((address_space(3))) void *)(dst + (wave * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ob + (tail ? offOt[i] : offO[i])),
                                             (__attribute__((address_space(3))) void *)(dst + kTile + (wave * 2 + i) * 1024), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(sb + (tail ? offSt : offS)),
                                         (__attribute__((address_space(3))) void *)(dst + 2 * kTile + wave * 256), 4, 0, 0);
    };
    issue_step(0, 0);
    issue_step(min(1, n_steps - 1), 1);
    asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    __syncthreads();
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    unsigned trA[D / 32], trB[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db) { trA[db] = lds0 + tr_off_u(db, lr, h, 0); trB[db] = lds0 + tr_off_u(db, lr, h, 8); }
    const unsigned statA = lds0 + 2 * kTile + 16 * h;        // + 32 g4 + 128 qb: the lane's four runs of four queries
    for (int step = 0; step < n_steps; ++step) {
        issue_step(min(step + 2, n_steps - 1), (step + 2) % 3);
        const int buf = step % 3;
        const unsigned char *lds_q = smem + buf * kStep, *lds_do = lds_q + kTile;
        const unsigned img = (unsigned)(buf * kStep);
        const int t0 = t_begin + (step % tiles_per_head) * 64;
        if (t0 + 63 >= wave_kmin) {                            // else: every query of the tile precedes every key of this wave
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < D / 16; ++ks) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain_u(lds_q, qb * 32 + lr, ks, h), kf[ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_plain_u(lds_do, qb * 32 + lr, ks, h), vf[ks], dp, 0, 0, 0);
                }
                // statistics and the transposed fragments of this query half: read (and waited for) under the products above
                f4v lse4[4], dl4[4];
                bf16x8 qtf[2][2], dotf[2][2];                // [s2][db]
                if (qb == 0) {
                    lds_rows4_wait<0>(lse4, statA + img);
                    lds_rows4_wait<256>(dl4, statA + img);
                    tr_frags4_wait<kTile, kTile + 16 * 128>(dotf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                    tr_frags4_wait<0, 16 * 128>(qtf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                } else {
                    lds_rows4_wait<128>(lse4, statA + img);
                    lds_rows4_wait<256 + 128>(dl4, statA + img);
                    tr_frags4_wait<kTile + 32 * 128, kTile + 48 * 128>(dotf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                    tr_frags4_wait<32 * 128, 48 * 128>(qtf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                }
                float pr[16], ds[16];
                const int qrel = t0 + 4 * h - vis_lo;                            // (query of element (g4, t)) - vis_lo = qrel + 32 qb + 8 g4 + t
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int r = 4 * g4 + t;
                        const bool vis = (unsigned)(qrel + (qb * 32 + 8 * g4 + t)) < vis_n;
                        const float e = vis ? fast_exp2(__builtin_fmaf(s[r], sc, -lse4[g4][t])) : 0.f;
                        pr[r] = e;
                        ds[r] = e * (dp[r] - dl4[g4][t]);                        // the softmax scale multiplies dK once, at the store
                    }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 pf = frag_from_acc(&pr[8 * s2]);
                    const bf16x8 dsf = frag_from_acc(&ds[8 * s2]);
#pragma unroll
                    for (int db = 0; db < D / 32; ++db) {
                        accV[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf[s2][db], pf, accV[db], 0, 0, 0);
                        accK[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[s2][db], dsf, accK[db], 0, 0, 0);
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");     // this wave's pieces of step + 1 have landed (step + 2's five may still fly)
        __builtin_amdgcn_s_barrier();                        // ... and everybody else's; all reads of this step's images are done
    }
    store_accT<D / 32>(accK, A.dk + (long long)g * D, A.lddk, rowbase + ki, kvalid, h, A.scale);
    store_accT<D / 32>(accV, A.dv + (long long)g * D, A.lddv, rowbase + ki, kvalid, h, 1.f);
}

// =====================================================================================================
// Round 3: the head_dim-64 kernels again, with the softmax arithmetic moved into the MFMA accumulators ("lean" kernels, g_attn_dma == 2).
// The LDS-DMA kernels above are vector-issue bound, not MFMA bound (ISA count of attn_fwd_kernel<64, true>: ~200 vector instructions beside 16
// MFMAs per 32 x 64 tile = ~930 issue cycles against 512 of MFMA; dK/dV 211 beside 32).  What a score costs besides its exp is removed:
//   * the row operand held in registers is PRE-SCALED by scale * log2(e) (rounded to bf16 once per row, as the persistent-workgroup attention of the
//     CDNA guide does): the products are log2-domain scores, no multiply per score;
//   * the row constant of the softmax is the INITIAL ACCUMULATOR of the score product (MFMA takes C != D): forward -- minus the row's running
//     maximum, so p = exp2(acc) with no subtraction; backward -- the row's log-sum-exp with the register operand negated, acc = lse - s, p = exp2(-acc)
//     (the negation is the instruction's source modifier); dP starts from delta the same way: acc = delta - dP, and ds = -(p * acc): one multiply, the
//     sign goes into the scale applied once at the store;
//   * forward: the running maximum is DEFERRED (T13 of the guide).  A tile takes the fast path -- no maximum at all, 32 exp + 32 adds + 16 packs --
//     unless some row has not seen a key yet or some lane's tile sum exceeds 2^10 (a score more than ~2^5..2^10 above the row's reference);
//     then the exact path: row maximum, rescale of l and O, new reference.  Tiles that need the causal / padding mask always take the exact path.
// The bf16 rounding points of P and dS are the ones of the kernels above; what changes is the rounding of the pre-scaled operand (half an ulp
// of bf16 on q resp. k: the size of the input's own quantisation) and the order of the fp32 sums inside the MFMA.  lse / delta keep their meaning
// and layout, so every lean kernel can be mixed with the others (tests A/B each one alone) -- up to the pre-scaled operand's rounding: a lean lse
// and exact scores (or the dK / dV kernel's pre-scaled k) disagree by up to 2^-8 of sum |q k| * scale * log2 e, which matters at large scores.
// =====================================================================================================

// row operand fragments, pre-scaled: bf16(x * mul) (mul = +-scale * log2 e, or -1 for a sign flip, which is exact)
__device__ __forceinline__ void scale_row_frags(bf16x8 (&f)[4], float mul)
{
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        using u4 = __attribute__((ext_vector_type(4))) unsigned;
        u4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = pack_bf16(bf2f((unsigned short)f[ks][2 * j]) * mul, bf2f((unsigned short)f[ks][2 * j + 1]) * mul);
        f[ks] = __builtin_bit_cast(bf16x8, w);
    }
}
// the fragments negated (exact: the sign bit of each bf16): one XOR per dword where scale_row_frags(f, -1.f) spent an unpack, a multiply and a pack on every pair
__device__ __forceinline__ void negate_row_frags(bf16x8 (&f)[4])
{
    using u4 = __attribute__((ext_vector_type(4))) unsigned;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u4, f[ks]) ^ 0x80008000u);
}

#ifndef ECGB_LEAN_DIAG
#define ECGB_LEAN_DIAG 0      // timing-only diagnostics of the forward kernel (wrong results): 1 no tile DMA in the loop, 2 no barrier, 4 no exp, 8 two of the eight P.V MFMAs, 16 four of the eight Q.K MFMAs, 32 no row sum
#endif
#ifndef ECGB_LEAN_FWD_WGS
#define ECGB_LEAN_FWD_WGS 3      // waves per SIMD the forward kernel is compiled for (168 registers; 2: 206).  Three: -9 ... -14 % (see the kernel)
#endif
#ifndef ECGB_LEAN_DQ_WGS
#define ECGB_LEAN_DQ_WGS 2
#endif
#ifndef ECGB_LEAN_DKV_WGS
#define ECGB_LEAN_DKV_WGS 2
#endif
#ifndef ECGB_LEAN_PRIO
#define ECGB_LEAN_PRIO 0      // 1: s_setprio 1 around the forward kernel's MFMA clusters (measured: no change, 0.248 against 0.250 ms)
#endif
#if ECGB_LEAN_PRIO
#define LEAN_PRIO(p) __builtin_amdgcn_s_setprio(p)
#else
#define LEAN_PRIO(p) do { } while (0)
#endif
constexpr int kLeanRing = 3;      // LDS ring depth of the lean kernels: tiles (kRing - 1) ahead (4 measured the same as 3: the flight time is not what a wave waits for)
template <int N> __device__ __forceinline__ void lean_wait_tiles() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }


// NW waves per workgroup (4 or 8) share every K / V tile.  Measured with the phase timers (scripts/dev_prof_attn.py, 4 waves x 32 rows, two workgroups per CU):
// 2 030 of a tile's 4 700 cycles went into ISSUING its four LDS-DMA pieces -- the vector memory path of a CU takes about 16 bytes per cycle, 32 KB per pair of
// workgroup tiles against 1 024 cycles of MFMA: the kernel was bound by the tile traffic, not by arithmetic.  So a tile serves twice the rows: eight waves,
// and -- grouped-query attention -- the waves of a workgroup are the HW = gcd(G, 8) query heads of the KV group times 8 / HW blocks of 32 rows (Llama: 4 heads
// x 64 rows, where both row blocks need exactly the same tiles: no wave idles at a barrier under the causal mask; one head: 256 rows).
template <int NW>
__global__ __launch_bounds__(NW * 64, ECGB_LEAN_FWD_WGS) void attn_fwd_lean_kernel(AttnArgs A)
{
    constexpr int D = 64, kTile = 128 * D, PPW = 8 / NW;      // PPW: 1 KiB pieces of a tile per wave and operand
    // Ring of kRing (K, V) tile pairs, kAhead = kRing - 1 tiles in flight, issued FIRST thing in a tile.  Measured (scripts/dev_attn_lean.py, C3 shape):
    // issuing tile it + 2 in the middle of tile it (in the vector-only stretch, where the guide prices an LDS-DMA issue lowest) cost 15 % of the kernel; a ring of
    // four (three tiles ahead) measured the same as three.
    constexpr int kRing = kLeanRing, kAhead = kRing - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // kRing x (K, V) tiles + the row's key mask
    float *lds_maskrow = reinterpret_cast<float *>(smem + 2 * kRing * kTile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    const int hw_log2 = A.lean_hw_log2, R = (NW >> hw_log2) * 32;          // heads per workgroup (log2), query rows per workgroup
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + R - 1) / R, (A.Hq / A.Hkv) >> hw_log2, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + (head_in << hw_log2) + (wave & ((1 << hw_log2) - 1));
    const int q0 = qblk * R, qw0 = q0 + (wave >> hw_log2) * 32;            // first row of the workgroup / of this wave
    const int qi = qw0 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    const int k_end = min(A.S, q0 + R);
    const int wave_qmax = qw0 + 31;
    const int last_tile = (k_end - 1) / 64;
    unsigned offK[PPW], offV[PPW], offKt[PPW], offVt[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave * PPW + i) * 8 + (lane >> 3), slot = lane & 7;
        const int ck = slot ^ ((r >> 1) & 7), cv = slot ^ (((r >> 1) & 1) << 2);
        const int rt = min(r, A.S - 1 - last_tile * 64);
        offK[i] = (unsigned)(((long long)r * A.ldk + ck * 8) * 2);  offKt[i] = (unsigned)(((long long)rt * A.ldk + ck * 8) * 2);
        offV[i] = (unsigned)(((long long)r * A.ldv + cv * 8) * 2);  offVt[i] = (unsigned)(((long long)rt * A.ldv + cv * 8) * 2);
    }
    // The tile stream as RUNNING state (round 4): the next tile's global bases, its index and its ring slot advance by adds.  Formed from the tile index every trip
    // (64-bit multiplies, a division by the ring depth) the issue was 50 scalar instructions per trip, a fifth of the trip's instruction count -- and a wave issues
    // one instruction per ~4.5 cycles whatever its kind.  UNCONDITIONAL (past the last tile the last one is issued again): the waits below stay counted.
    const unsigned char *kb_next = reinterpret_cast<const unsigned char *>(K + rowbase * A.ldk), *vb_next = reinterpret_cast<const unsigned char *>(V + rowbase * A.ldv);
    const long long stepK = 128ll * A.ldk, stepV = 128ll * A.ldv;       // bytes from one 64-key tile to the next
    const bool tail_last = (last_tile + 1) * 64 > A.S;
    int t_next = 0;
    unsigned slot_next = 0;                                             // byte offset of the ring slot the next tile lands in
    auto issue_next = [&]() {
        const bool tail = tail_last && t_next == last_tile;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            unsigned ok = offK[i], ov = offV[i];
            if (tail) {                                          // (uniform, the one partial tile a sequence can end with) rows past the last key re-read it
                const int r = (wave * PPW + i) * 8 + (lane >> 3), slot = lane & 7, rt = min(r, A.S - 1 - last_tile * 64);
                ok = (unsigned)(((long long)rt * A.ldk + (slot ^ ((r >> 1) & 7)) * 8) * 2);
                ov = (unsigned)(((long long)rt * A.ldv + (slot ^ (((r >> 1) & 1) << 2)) * 8) * 2);
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb_next + ok),
                                             (__attribute__((address_space(3))) void *)(smem + slot_next + (wave * PPW + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb_next + ov),
                                             (__attribute__((address_space(3))) void *)(smem + slot_next + kTile + (wave * PPW + i) * 1024), 16, 0, 0);
        }
        if (t_next < last_tile) { ++t_next; kb_next += stepK; vb_next += stepV; }
        slot_next = slot_next == (kRing - 1) * 2 * kTile ? 0u : slot_next + 2 * kTile;
    };
#pragma unroll
    for (int t = 0; t < kAhead; ++t) issue_next();
    bf16x8 qf[4];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // Q's fragments (younger than the tiles' pieces) are in: from here on the waits are counted
    scale_row_frags(qf, A.scale * kLog2e);                   // log2-domain scores straight out of the MFMA
    lean_fill_mask<NW>(lds_maskrow, A.mask + rowbase, A.S, (k_end + 63) & ~63);
    f32x16 accO[2] = {splat16(0.f), splat16(0.f)};
    float m = -INFINITY, l = 0.f;                            // m: the row's reference (a deferred running maximum); -inf = no key seen yet
    f32x16 cinit = splat16(0.f);                             // -m in all sixteen registers: the initial accumulator of the score products
    __syncthreads();
    const unsigned long long padbits = lean_pad_bits(lds_maskrow, (k_end + 63) & ~63);
    unsigned vtr[2];
    {
        const int a = lr >> 4, q = (lr & 15) >> 2, p = lr & 3;
        const int key = 4 * h + q;
#pragma unroll
        for (int db = 0; db < 2; ++db)
            vtr[db] = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem + kTile + key * 128 +
                      (((db * 4 + 2 * a + (p >> 1)) ^ (((key >> 1) & 1) << 2)) << 4) + (p & 1) * 8;
    }
    const unsigned lds_base_u = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    unsigned kbase[4];                                       // this lane's K row fragment (key lr, k-step ks) inside a K image; key 32 + lr is 4 KiB further
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        kbase[ks] = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem + lr * 128 + (((ks * 2 + h) ^ ((lr >> 1) & 7)) << 4);
#ifdef ECGB_PROFILE
    unsigned long long prof_acc[7] = {};
    long long t_prof = clock64();
#endif
    unsigned vimg = 0;                                       // byte offset of the ring slot of the current tile
    for (int k0 = 0, it = 0; k0 < k_end; k0 += 64, ++it) {
        const float *lds_mask = lds_maskrow + k0;
#if !(ECGB_LEAN_DIAG & 1)
        issue_next();                                        // FIRST thing in the tile: the pieces need their whole flight time (see kRing)
#endif
        APROF(0);
        if (k0 <= wave_qmax) {
            const bool need_mask = (k0 + 63 > qw0) || lean_tile_padded(padbits, it);
            f32x16 sacc[2];
            bf16x8 kfr[2][4];                                   // [kb][ks]: K row fragments, four per batch; the second batch and the V^T fragments land under MFMAs
            const unsigned kb0 = (unsigned)(lr * 128 + ((h ^ ((lr >> 1) & 7)) << 4)), kl0 = lds_base_u + vimg;      // k-step ks is the offset ^ (ks << 5): recomputed, not held
            lds_frags2x2_wait<0, 4096>(kfr[0][0], kfr[1][0], kfr[0][1], kfr[1][1], kb0 + kl0, (kb0 ^ 32u) + kl0);
            LEAN_PRIO(1);
            sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0][0], qf[0], cinit, 0, 0, 0);
            sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[1][0], qf[0], cinit, 0, 0, 0);
            sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0][1], qf[1], sacc[0], 0, 0, 0);
            sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[1][1], qf[1], sacc[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            lds_frags2x2_wait<0, 4096>(kfr[0][2], kfr[1][2], kfr[0][3], kfr[1][3], (kb0 ^ 64u) + kl0, (kb0 ^ 96u) + kl0);
#if !(ECGB_LEAN_DIAG & 16)
#pragma unroll
            for (int ks = 2; ks < 4; ++ks)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[kb][ks], qf[ks], sacc[kb], 0, 0, 0);
#endif
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 vfr[2][2][2];                                // [kb][s2][db]: the tile's eight V^T fragments
            APROF(1);
            LEAN_PRIO(0);
            bf16x8 pf[2][2];                                    // [kb][s2]: P as the B operand of P.V, packed as it is produced (the fp32 values are not kept)
            using u4 = __attribute__((ext_vector_type(4))) unsigned;
            bool exact = need_mask;
            if (!need_mask) {                                   // (uniform) fast path: p = exp2(score - reference) is the accumulator's exp2
                // the row sum as FOUR chains of eight adds (one per fragment of P): as one chain of 32 dependent adds it was 13 % of the kernel -- with two waves
                // per SIMD nothing else of this wave can issue behind an add that waits for the previous one
                float ls[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        u4 w;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
#if ECGB_LEAN_DIAG & 4
                            const float e0 = sacc[kb][8 * s2 + 2 * j], e1 = sacc[kb][8 * s2 + 2 * j + 1];
#else
                            const float e0 = fast_exp2(sacc[kb][8 * s2 + 2 * j]), e1 = fast_exp2(sacc[kb][8 * s2 + 2 * j + 1]);
#endif
#if !(ECGB_LEAN_DIAG & 32)
                            ls[kb][s2] += e0; ls[kb][s2] += e1;
#endif
                            w[j] = pack_bf16(e0, e1);
                        }
                        pf[kb][s2] = __builtin_bit_cast(bf16x8, w);
                    }
                const float lsum = (ls[0][0] + ls[0][1]) + (ls[1][0] + ls[1][1]);
                // not (lsum <= 2^10) also catches +inf; a row that has seen no key yet has no reference: exact path
                exact = __any(!(lsum <= 1024.f) || m == -INFINITY);
                if (!exact) l += lsum;
            }
            if (exact) {
                float t = -INFINITY;
                if (need_mask) {
                    f4v mv[2][4];
                    const unsigned ma = (unsigned)(size_t)(__attribute__((address_space(3))) float *)const_cast<float *>(lds_mask) + 16 * h;
                    lds_rows4_wait<0>(mv[0], ma);
                    lds_rows4_wait<128>(mv[1], ma);
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // key inside the tile
                            const bool vis = (k0 + kl <= qi) & (mv[kb][r >> 2][r & 3] != 0.f);
                            const float v = vis ? sacc[kb][r] : -INFINITY;
                            sacc[kb][r] = v;
                            t = fmaxf(t, v);
                        }
                } else {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) t = fmaxf(t, sacc[kb][r]);
                }
                t = fmaxf(t, __shfl_xor(t, 32, 64));            // the row's maximum of (score - reference); -inf: no visible key in this tile
                // unseen row: the reference becomes the tile's maximum itself (if there is one); seen row: it only ever moves up
                const bool unseen = m == -INFINITY;
                const float d = (t == -INFINITY) ? 0.f : (unseen ? t : fmaxf(t, 0.f));
                const float alpha = unseen ? 1.f : fast_exp2(-d);   // (an unseen row's l and O are still zero)
                float ls[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        u4 w;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float e0 = fast_exp2(sacc[kb][8 * s2 + 2 * j] - d), e1 = fast_exp2(sacc[kb][8 * s2 + 2 * j + 1] - d);
                            ls[kb][s2] += e0; ls[kb][s2] += e1;
                            w[j] = pack_bf16(e0, e1);
                        }
                        pf[kb][s2] = __builtin_bit_cast(bf16x8, w);
                    }
                const float lsum = (ls[0][0] + ls[0][1]) + (ls[1][0] + ls[1][1]);
                l = l * alpha + lsum;
                if (t != -INFINITY) m = unseen ? t : m + d;
                if (__any(alpha != 1.f)) {
#pragma unroll
                    for (int db = 0; db < 2; ++db)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accO[db][r] *= alpha;
                }
                if (__any(d != 0.f)) cinit = splat16(m == -INFINITY ? 0.f : -m);
            }
            APROF(2);
            LEAN_PRIO(1);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (kb == 0) tr_frags4_wait<0, 16 * 128>(vfr[0], vtr[0] + vimg, vtr[0] + vimg + 1024, vtr[1] + vimg, vtr[1] + vimg + 1024);
                else tr_frags4_wait<32 * 128, 48 * 128>(vfr[0], vtr[0] + vimg, vtr[0] + vimg + 1024, vtr[1] + vimg, vtr[1] + vimg + 1024);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int db = 0; db < 2; ++db)
                        accO[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0][s2][db], pf[kb][s2], accO[db], 0, 0, 0);
            }
            LEAN_PRIO(0);
            APROF(3);
        }
#if !(ECGB_LEAN_DIAG & 1)
        lean_wait_tiles<2 * PPW * (kAhead - 1)>();         // this wave's pieces of tile it + 1 have landed (the younger tiles' may still fly)
#endif
        APROF(4);
#if !(ECGB_LEAN_DIAG & 2)
        __builtin_amdgcn_s_barrier();                      // ... and everybody else's; all reads of tile it are done
#endif
        vimg = vimg == (kRing - 1) * 2 * kTile ? 0u : vimg + 2 * kTile;
        APROF(5);
#ifdef ECGB_PROFILE
        prof_acc[6] += 1;
#endif
    }
#ifdef ECGB_PROFILE
    if ((threadIdx.x & 63) == 0)
        for (int kk = 0; kk < 7; ++kk) atomicAdd(&g_attn_prof[(threadIdx.x >> 6) * 8 + kk], prof_acc[kk]);
#endif
    const float lt = l + __shfl_xor(l, 32, 64);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    store_accT<2>(accO, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h, inv);
    if (qvalid && h == 0) A.lse[((long long)b * A.Hq + hq) * A.S + qi] = lt > 0.f ? m + log2f(lt) : INFINITY;
}

// dQ, lean form: lanes = queries.  Register operands: -Q * scale * log2 e and -dO; initial accumulators: the row's lse and delta.
//   acc_s = lse - s,  p = exp2(-acc_s);   acc_dp = delta - dP;   dsn = p * acc_dp = -dS;   accQ += K^T . dsn  ->  dQ = -scale * accQ
template <int NW>
__global__ __launch_bounds__(NW * 64, ECGB_LEAN_DQ_WGS) void attn_bwd_dq_lean_kernel(AttnArgs A)
{
    constexpr int D = 64, kTile = 128 * D, PPW = 8 / NW;      // (waves, heads and rows of a workgroup: see attn_fwd_lean_kernel)
    constexpr int kRing = kLeanRing, kAhead = kRing - 1;   // (see attn_fwd_lean_kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // kRing x (K, V) + 4 bytes per key
    float *lds_maskrow = reinterpret_cast<float *>(smem + 2 * kRing * kTile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    const int hw_log2 = A.lean_hw_log2, R = (NW >> hw_log2) * 32;
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + R - 1) / R, (A.Hq / A.Hkv) >> hw_log2, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + (head_in << hw_log2) + (wave & ((1 << hw_log2) - 1));
    const int q0 = qblk * R, qw0 = q0 + (wave >> hw_log2) * 32;
    const int qi = qw0 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    const int k_end = min(A.S, q0 + R);
    const int wave_qmax = qw0 + 31;
    const int last_tile = (k_end - 1) / 64;
    unsigned offK[PPW], offV[PPW], offKt[PPW], offVt[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave * PPW + i) * 8 + (lane >> 3), c = (lane & 7) ^ swz_u(r);
        const int rt = min(r, A.S - 1 - last_tile * 64);
        offK[i] = (unsigned)(((long long)r * A.ldk + c * 8) * 2);  offKt[i] = (unsigned)(((long long)rt * A.ldk + c * 8) * 2);
        offV[i] = (unsigned)(((long long)r * A.ldv + c * 8) * 2);  offVt[i] = (unsigned)(((long long)rt * A.ldv + c * 8) * 2);
    }
    // (the tile stream as running state: see attn_fwd_lean_kernel)
    const unsigned char *kb_next = reinterpret_cast<const unsigned char *>(K + rowbase * A.ldk), *vb_next = reinterpret_cast<const unsigned char *>(V + rowbase * A.ldv);
    const long long stepK = 128ll * A.ldk, stepV = 128ll * A.ldv;       // bytes from one 64-key tile to the next
    const bool tail_last = (last_tile + 1) * 64 > A.S;
    int t_next = 0;
    unsigned slot_next = 0;                                             // byte offset of the ring slot the next tile lands in
    auto issue_next = [&]() {
        const bool tail = tail_last && t_next == last_tile;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb_next + (tail ? offKt[i] : offK[i])),
                                             (__attribute__((address_space(3))) void *)(smem + slot_next + (wave * PPW + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb_next + (tail ? offVt[i] : offV[i])),
                                             (__attribute__((address_space(3))) void *)(smem + slot_next + kTile + (wave * PPW + i) * 1024), 16, 0, 0);
        }
        if (t_next < last_tile) { ++t_next; kb_next += stepK; vb_next += stepV; }
        slot_next = slot_next == (kRing - 1) * 2 * kTile ? 0u : slot_next + 2 * kTile;
    };
#pragma unroll
    for (int t = 0; t < kAhead; ++t) issue_next();
    bf16x8 qf[4], dof[4], of[4];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    load_row_frags<D>(dof, A.d_o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    load_row_frags<D>(of, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h);
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += bf2f((unsigned short)dof[ks][j]) * bf2f((unsigned short)of[ks][j]);
    delta += __shfl_xor(delta, 32, 64);
    const long long stat = ((long long)b * A.Hq + hq) * A.S + qi;
    if (qvalid && h == 0) A.delta[stat] = delta;
    const float lse = qvalid ? A.lse[stat] : INFINITY;
    scale_row_frags(qf, -A.scale * kLog2e);
    negate_row_frags(dof);
    const f32x16 lseC = splat16(lse), delC = splat16(delta);
    f32x16 accQ[2] = {splat16(0.f), splat16(0.f)};
    lean_fill_mask<NW>(lds_maskrow, A.mask + rowbase, A.S, (k_end + 63) & ~63);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (the row loads above are younger than the tiles' pieces: one full wait, once)
    __syncthreads();
    const unsigned long long padbits = lean_pad_bits(lds_maskrow, (k_end + 63) & ~63);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    unsigned trA[2], trB[2];
#pragma unroll
    for (int db = 0; db < 2; ++db) { trA[db] = lds0 + tr_off_u(db, lr, h, 0); trB[db] = lds0 + tr_off_u(db, lr, h, 8); }
    unsigned rbase[4];                                       // this lane's row fragment (row lr, k-step ks) inside an image; row 32 + lr is 4 KiB further
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rbase[ks] = lds0 + lr * 128 + (((ks * 2 + h) ^ swz_u(lr)) << 4);
    unsigned kimg = 0;                                       // byte offset of the ring slot of the current tile
    for (int k0 = 0, it = 0; k0 < k_end; k0 += 64, ++it) {
        issue_next();
        if (k0 <= wave_qmax) {
            const float *lds_mask = lds_maskrow + k0;
            const bool need_mask = (k0 + 63 > qw0) || lean_tile_padded(padbits, it);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                bf16x8 kfr[4], vfr[4];                        // row fragments of this key half: K and V images side by side (+ kTile), two k-steps per batch
                if (kb == 0) lds_frags2x2_wait<0, kTile>(kfr[0], vfr[0], kfr[1], vfr[1], rbase[0] + kimg, rbase[1] + kimg);
                else lds_frags2x2_wait<4096, kTile + 4096>(kfr[0], vfr[0], kfr[1], vfr[1], rbase[0] + kimg, rbase[1] + kimg);
                f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0], qf[0], lseC, 0, 0, 0);
                f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0], dof[0], delC, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[1], qf[1], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[1], dof[1], dp, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kb == 0) lds_frags2x2_wait<0, kTile>(kfr[2], vfr[2], kfr[3], vfr[3], rbase[2] + kimg, rbase[3] + kimg);
                else lds_frags2x2_wait<4096, kTile + 4096>(kfr[2], vfr[2], kfr[3], vfr[3], rbase[2] + kimg, rbase[3] + kimg);
#pragma unroll
                for (int ks = 2; ks < 4; ++ks) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[ks], qf[ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[ks], dof[ks], dp, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                bf16x8 ktf[2][2];
                if (kb == 0) tr_frags4_wait<0, 16 * 128>(ktf, trA[0] + kimg, trB[0] + kimg, trA[1] + kimg, trB[1] + kimg);
                else tr_frags4_wait<32 * 128, 48 * 128>(ktf, trA[0] + kimg, trB[0] + kimg, trA[1] + kimg, trB[1] + kimg);
                float ds[16];
                if (need_mask) {
                    f4v mv[4];
                    const unsigned ma = (unsigned)(size_t)(__attribute__((address_space(3))) float *)const_cast<float *>(lds_mask) + 16 * h;
                    if (kb == 0) lds_rows4_wait<0>(mv, ma); else lds_rows4_wait<128>(mv, ma);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const bool vis = (k0 + kl <= qi) & (mv[r >> 2][r & 3] != 0.f);
                        ds[r] = vis ? fast_exp2(-s[r]) * dp[r] : 0.f;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(-s[r]) * dp[r];
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 dsf = frag_from_acc(&ds[8 * s2]);
#pragma unroll
                    for (int db = 0; db < 2; ++db)
                        accQ[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf[s2][db], dsf, accQ[db], 0, 0, 0);
                }
            }
        }
        lean_wait_tiles<2 * PPW * (kAhead - 1)>();
        __builtin_amdgcn_s_barrier();
        kimg = kimg == (kRing - 1) * 2 * kTile ? 0u : kimg + 2 * kTile;
    }
    if (A.rope_cos) store_accT_rope_inv(accQ, A.dq + (long long)hq * D, A.lddq, rowbase + qi, qvalid, h, -A.scale, A.rope_cos + (rowbase + qi) * 32, A.rope_sin + (rowbase + qi) * 32);
    else store_accT<2>(accQ, A.dq + (long long)hq * D, A.lddq, rowbase + qi, qvalid, h, -A.scale);
}

// dK / dV, lean form: lanes = keys.  Register operands: -K * scale * log2 e and -V; initial accumulators: the tile's lse / delta rows as they lie in LDS
// (the lane's sixteen queries are four runs of four floats: four 16-byte reads ARE the sixteen accumulator registers).
//   acc_s = lse_q - s,  p = exp2(-acc_s);  acc_dp = delta_q - dP;  dsn = p * acc_dp = -dS;  accV += dO^T . p;  accK += Q^T . dsn  ->  dK = -scale * accK
// NW waves = NW x 32 keys per workgroup share every (Q, dO) tile (see attn_fwd_lean_kernel: the tile traffic, not the arithmetic, bounds the 4-wave kernel).
template <int NW>
__global__ __launch_bounds__(NW * 64, ECGB_LEAN_DKV_WGS) void attn_bwd_dkv_lean_kernel(AttnArgs A)
{
    constexpr int D = 64, kTile = 128 * D, PPW = 8 / NW, kStep = 2 * kTile + NW * 256;      // Q image, dO image, one 256-byte statistics row per wave
    constexpr int kRing = kLeanRing, kAhead = kRing - 1;   // (see attn_fwd_lean_kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // kRing x kStep
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    // Under the causal mask key block j of a sequence has (n_blk - j) x as many query tiles as the last one: with one block per workgroup the 2 048 workgroups of the C3
    // shape carry 8 .. 64 steps each and the 512 slots of the chip were 58 % used (phase timers: 3 680 cycles per step and wave, 73 728 steps, 453 us).  A workgroup takes
    // the PAIR (j, n_blk - 1 - j): every workgroup the same work.
    const int n_blk = (A.S + NW * 32 - 1) / (NW * 32);
    int pair, head_in, group;
    map_block((int)blockIdx.x, (n_blk + 1) / 2, 1, A.B * A.Hkv, false, pair, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv;
    const int G = A.Hq / A.Hkv;
    for (int half = 0; half < 2; ++half) {
    const int blk = half == 0 ? pair : n_blk - 1 - pair;
    if (half == 1) {
        if (blk == pair) break;                              // an odd number of blocks: the middle one once
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the clamped re-issues of the last step may still be landing in the ring
        __syncthreads();
    }
    const int kk0 = blk * (NW * 32);
    const int ki = kk0 + wave * 32 + lr;
    const bool kvalid = ki < A.S;
    const long long rowbase = (long long)b * A.S;
    const int wave_kmin = kk0 + wave * 32;
    const int t_begin = (kk0 / 64) * 64;
    const int tiles_per_head = (A.S - t_begin + 63) / 64;
    const int n_steps = G * tiles_per_head;
    const int tail_rows = A.S - (t_begin + (tiles_per_head - 1) * 64);
    unsigned offQ[PPW], offO[PPW], offQt[PPW], offOt[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave * PPW + i) * 8 + (lane >> 3), c = (lane & 7) ^ swz_u(r);
        const int rt = min(r, tail_rows - 1);
        offQ[i] = (unsigned)(((long long)r * A.ldq + c * 8) * 2);  offQt[i] = (unsigned)(((long long)rt * A.ldq + c * 8) * 2);
        offO[i] = (unsigned)(((long long)r * A.ldo + c * 8) * 2);  offOt[i] = (unsigned)(((long long)rt * A.ldo + c * 8) * 2);
    }
    const unsigned offS = (unsigned)lane * 4u, offSt = (unsigned)min(lane, tail_rows - 1) * 4u;
    const float *stat_src = (wave & 1) ? A.delta : A.lse;
    auto issue_step = [&](int step, int buf) {
        const int hq = g * G + step / tiles_per_head;
        const int ti = step % tiles_per_head;
        const int t0 = t_begin + ti * 64;
        const bool tail = ti == tiles_per_head - 1 && tail_rows < 64;
        const unsigned char *qb = reinterpret_cast<const unsigned char *>(A.q + (long long)hq * D + (rowbase + t0) * A.ldq);
        const unsigned char *ob = reinterpret_cast<const unsigned char *>(A.d_o + (long long)hq * D + (rowbase + t0) * A.ldo);
        const unsigned char *sb = reinterpret_cast<const unsigned char *>(stat_src + ((long long)b * A.Hq + hq) * A.S + t0);
        unsigned char *dst = smem + buf * kStep;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + (tail ? offQt[i] : offQ[i])),
                                             (__attribute__((address_space(3))) void *)(dst + (wave * PPW + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ob + (tail ? offOt[i] : offO[i])),
                                             (__attribute__((address_space(3))) void *)(dst + kTile + (wave * PPW + i) * 1024), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(sb + (tail ? offSt : offS)),
                                         (__attribute__((address_space(3))) void *)(dst + 2 * kTile + wave * 256), 4, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < kAhead; ++t) issue_step(min(t, n_steps - 1), t);
    bf16x8 kf[4], vf[4];
    load_row_frags<D>(kf, A.k + (long long)g * D, A.ldk, rowbase + ki, kvalid, h);
    load_row_frags<D>(vf, A.v + (long long)g * D, A.ldv, rowbase + ki, kvalid, h);
    const bool kvis = kvalid && A.mask[rowbase + (kvalid ? ki : 0)] != 0.f;
    scale_row_frags(kf, -A.scale * kLog2e);
    negate_row_frags(vf);
    const int vis_lo = kvis ? ki : A.S;
    const unsigned vis_n = (unsigned)(A.S - vis_lo);
    const bool wave_all_keys = __all(kvis);                  // (uniform) no padded / out-of-range key among this wave's 32
    f32x16 accK[2] = {splat16(0.f), splat16(0.f)}, accV[2] = {splat16(0.f), splat16(0.f)};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (the row loads above are younger than the steps' pieces: one full wait, once)
    __syncthreads();
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    unsigned trA[2], trB[2];
#pragma unroll
    for (int db = 0; db < 2; ++db) { trA[db] = lds0 + tr_off_u(db, lr, h, 0); trB[db] = lds0 + tr_off_u(db, lr, h, 8); }
    const unsigned statA = lds0 + 2 * kTile + 16 * h;        // + 32 g4 + 128 qb: the lane's four runs of four queries
    unsigned rbase[4];                                       // this lane's row fragment (row lr, k-step ks) inside an image; row 32 + lr is 4 KiB further
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rbase[ks] = lds0 + lr * 128 + (((ks * 2 + h) ^ swz_u(lr)) << 4);
#ifdef ECGB_PROFILE
    unsigned long long prof_acc[8] = {};
    long long t_prof = clock64();
#endif
    for (int step = 0; step < n_steps; ++step) {
        issue_step(min(step + kAhead, n_steps - 1), (step + kAhead) % kRing);
        APROF(0);
        const int buf = step % kRing;
        const unsigned img = (unsigned)(buf * kStep);
        const int t0 = t_begin + (step % tiles_per_head) * 64;
        if (t0 + 63 >= wave_kmin) {                            // else: every query of the tile precedes every key of this wave
            // (uniform) every (query, key) pair of this wave's 64 x 32 block is visible: queries all real and none before a key, keys all real
            const bool all_vis = wave_all_keys && t0 >= wave_kmin + 31 && t0 + 64 <= A.S;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                f4v lse4[4], dl4[4];
                bf16x8 qfr[4], ofr[4];                        // row fragments of this query half: Q and dO images side by side (+ kTile), two k-steps per batch
                if (qb == 0) lds_stats_frags_wait<0, 0, kTile>(lse4, dl4, qfr[0], ofr[0], qfr[1], ofr[1], statA + img, rbase[0] + img, rbase[1] + img);
                else lds_stats_frags_wait<128, 4096, kTile + 4096>(lse4, dl4, qfr[0], ofr[0], qfr[1], ofr[1], statA + img, rbase[0] + img, rbase[1] + img);
                APROF(1);
                f32x16 c_s = __builtin_shufflevector(__builtin_shufflevector(lse4[0], lse4[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                                     __builtin_shufflevector(lse4[2], lse4[3], 0, 1, 2, 3, 4, 5, 6, 7),
                                                     0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                const f32x16 c_dp = __builtin_shufflevector(__builtin_shufflevector(dl4[0], dl4[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                                            __builtin_shufflevector(dl4[2], dl4[3], 0, 1, 2, 3, 4, 5, 6, 7),
                                                            0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                if (!all_vis) {                               // an invisible pair starts from +inf: p = exp2(-inf) = 0 exactly
                    const int qrel = t0 + 4 * h - vis_lo;     // (query of element r) - vis_lo = qrel + 32 qb + 8 (r >> 2) + (r & 3)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        c_s[r] = ((unsigned)(qrel + (qb * 32 + 8 * (r >> 2) + (r & 3))) < vis_n) ? c_s[r] : INFINITY;
                }
                f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[0], kf[0], c_s, 0, 0, 0);
                f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ofr[0], vf[0], c_dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[1], kf[1], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ofr[1], vf[1], dp, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (qb == 0) lds_frags2x2_wait<0, kTile>(qfr[2], ofr[2], qfr[3], ofr[3], rbase[2] + img, rbase[3] + img);
                else lds_frags2x2_wait<4096, kTile + 4096>(qfr[2], ofr[2], qfr[3], ofr[3], rbase[2] + img, rbase[3] + img);
#pragma unroll
                for (int ks = 2; ks < 4; ++ks) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[ks], kf[ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ofr[ks], vf[ks], dp, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                float pr[16], ds[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e = fast_exp2(-s[r]);
                    pr[r] = e;
                    ds[r] = e * dp[r];
                }
                const bf16x8 pf0 = frag_from_acc(&pr[0]), pf1 = frag_from_acc(&pr[8]), dsf0 = frag_from_acc(&ds[0]), dsf1 = frag_from_acc(&ds[8]);
                APROF(2);
                {                                             // the transposed fragments one image at a time (dO, then Q): sixteen registers live instead of thirty-two
                    bf16x8 tf[2][2];                          // [s2][db]
                    if (qb == 0) tr_frags4_wait<kTile, kTile + 16 * 128>(tf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                    else tr_frags4_wait<kTile + 32 * 128, kTile + 48 * 128>(tf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        accV[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[0][db], pf0, accV[db], 0, 0, 0);
                        accV[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[1][db], pf1, accV[db], 0, 0, 0);
                    }
                    if (qb == 0) tr_frags4_wait<0, 16 * 128>(tf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
                    else tr_frags4_wait<32 * 128, 48 * 128>(tf, trA[0] + img, trB[0] + img, trA[1] + img, trB[1] + img);
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        accK[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[0][db], dsf0, accK[db], 0, 0, 0);
                        accK[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[1][db], dsf1, accK[db], 0, 0, 0);
                    }
                }
                APROF(3);
            }
        }
        lean_wait_tiles<(2 * PPW + 1) * (kAhead - 1)>();
        APROF(4);
        __builtin_amdgcn_s_barrier();
        APROF(5);
#ifdef ECGB_PROFILE
        prof_acc[6] += 1;
#endif
    }
#ifdef ECGB_PROFILE
    if ((threadIdx.x & 63) == 0)
        for (int kk = 0; kk < 7; ++kk) atomicAdd(&g_attn_prof[(threadIdx.x >> 6) * 8 + kk], prof_acc[kk]);
#endif
    if (A.rope_cos) store_accT_rope_inv(accK, A.dk + (long long)g * D, A.lddk, rowbase + ki, kvalid, h, -A.scale, A.rope_cos + (rowbase + ki) * 32, A.rope_sin + (rowbase + ki) * 32);
    else store_accT<2>(accK, A.dk + (long long)g * D, A.lddk, rowbase + ki, kvalid, h, -A.scale);
    store_accT<2>(accV, A.dv + (long long)g * D, A.lddv, rowbase + ki, kvalid, h, 1.f);
    }
}

template <int D, int DS, int WHICH = 0, bool DROP = false>
__global__ __launch_bounds__(256, D == 64 ? 2 : 1) void attn_bwd_dkv_kernel(AttnArgs A)   // head_dim 64: two waves per SIMD (<= 256 registers)
{
    int blk, head_in, group;
    map_block((int)blockIdx.x, ((A.S + 127) / 128) * DS, 1, A.B * A.Hkv, false, blk, head_in, group);   // key block 0 sees every query: first
    attn_bwd_dkv_body<D, DS, WHICH, DROP>(A, blk, group / A.Hkv, group % A.Hkv);
}
// head_dim 256: the dV pass and the dK pass of a key block as two workgroups of ONE launch (even / odd blockIdx.x) -- Gemma's single KV
// head gives only S / 128 x batch key blocks, half a chip's worth at C5's shape
template <int D>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv_pair_kernel(AttnArgs A)
{
    // blocks of a (batch, KV head) group: (key block, head split, pass) with the key block slowest -- heaviest first
    const int hs = A.head_splits > 1 ? A.head_splits : 1;
    int blk, head_in, group;
    map_block((int)blockIdx.x, ((A.S + 127) / 128) * 2 * hs, 1, A.B * A.Hkv, false, blk, head_in, group);
    const int pass = blk & 1, hsplit = (blk >> 1) % hs, kblk = (blk >> 1) / hs;
    if (pass) attn_bwd_dkv_body<D, 1, 2>(A, kblk, group / A.Hkv, group % A.Hkv, hsplit);
    else attn_bwd_dkv_body<D, 1, 1>(A, kblk, group / A.Hkv, group % A.Hkv, hsplit);
}

// dk / dv [row][g * D + d] (bf16, row strides lddk / lddv) = sum over the head splits of the fp32 slabs, in split order
template <int D>
__global__ __launch_bounds__(256) void attn_dkv_reduce_kernel(AttnArgs A)
{
    const long long rows_all = (long long)A.B * A.S, slab = rows_all * A.Hkv * D;
    const long long n4 = slab / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n4; i += (long long)gridDim.x * blockDim.x) {
        const int which = i >= n4;                           // 0 = dK, 1 = dV
        const long long e = (i - which * n4) * 4;            // element inside a slab: [g][row][d]
        const long long g = e / (rows_all * D), row = (e / D) % rows_all;
        const int d = (int)(e % D);
        using f4 = __attribute__((ext_vector_type(4))) float;
        f4 v = *reinterpret_cast<const f4 *>(A.slab + (long long)which * A.head_splits * slab + e);
        for (int hsp = 1; hsp < A.head_splits; ++hsp) v += *reinterpret_cast<const f4 *>(A.slab + ((long long)which * A.head_splits + hsp) * slab + e);
        using u2 = __attribute__((ext_vector_type(2))) unsigned;
        u2 o;
        o[0] = pack_bf16(v[0], v[1]); o[1] = pack_bf16(v[2], v[3]);
        unsigned short *dst = which ? A.dv + row * A.lddv : A.dk + row * A.lddk;
        *reinterpret_cast<u2 *>(dst + g * D + d) = o;
    }
}

// head_dim 64 forward and backward: 2 = the lean kernels (LDS-DMA staging, softmax constants in the MFMA accumulators: the default), 1 = the round-2 LDS-DMA
// kernels, 0 = the register-staged kernels (tests / A-B).  Bits 8 / 9 / 10 send the forward / dQ / dK-dV kernel alone back to mode 1 (A-B of one kernel).
int g_attn_dma = 2;
// head_dim 256 backward: 0 (default) = the pair kernel (the dK pass and the dV pass each form the scores), 1 = the dK pass hands its probabilities to a dV kernel through the
// scratch (ecgb_attn_bwd_scratch_bytes then asks for batch * heads * seq^2 bf16 more).  Measured at the C5 shape: 270 + 131 us against the pair's 447, 0.66 against 0.68 ms
// for the whole backward -- not worth a transient S x S tensor in HBM by default (ecgb_set_attn_d256_pass_p; the same bits either way)
int g_attn_d256_pass_p = 0;

// waves per workgroup of the lean kernels: 4 (default; two workgroups per CU) or 8 (one workgroup per CU, a K / V tile serves twice the rows: measured 15 %
// slower end to end at the C3 shape although its tile loop is faster -- scripts/experiments/r03_attn_fwd_pingpong.hip.txt; kept for A-B: ecgb_set_attn_lean_waves)
int g_lean_waves = 4;
// forward / dQ lean kernels: HW = gcd(G, waves) query heads of a KV group per workgroup (a power of two), waves / HW blocks of 32 rows
// =====================================================================================================
// Round 4: head_dim 256 (Gemma) forward with LDS-DMA staging.  The register-staged kernel above spends more than half of a tile's 10 800 cycles moving the tile
// (phase timers at the C5 shape: 2 530 issuing the next tile's loads into registers, 1 170 - 2 750 writing them to LDS -- the transposed V image most -- and up to 2 100
// at the barrier behind the slower half) and keeps its 128 output accumulators in the register file's upper half as spill space of the forced VGPR form (445 registers:
// a copy out and back around every product).  Here
//   * K and V tiles (64 keys x 512 bytes each) go global -> LDS by LDS-DMA, 1 KiB (two rows) per wave-instruction, eight pieces per wave and operand, one tile ahead
//     into a ring of two (a trip is > 4 000 cycles of MFMA: one tile of flight time is enough, and two stages are what 160 KB hold);
//   * K lies as rows with 16-byte chunk c of row r at c ^ (r & 15): the sixteen rows sixteen lanes read as fragments fall on sixteen different bank groups;
//     V lies as it is in memory ([key][d]) with its 64-byte group w of key row r at w ^ (r & 7): the P.V operand is gathered by transposing reads whose eight key rows
//     then cover eight different groups.  Both swizzles are applied on the global side of the DMA;
//   * all LDS reads are asm statements with their own wait (a read hipcc can see next to LDS-DMA gets a vmcnt(0) in front of it);
//   * without the staging registers the kernel needs 328 registers instead of 445: 72 values live in the upper half between uses instead of 189.  (The P.V products written
//     out as asm statements on "+a" accumulators kept all 128 there, ran at the same speed and were WRONG now and then in output columns 0..31 -- a wait-state rule between
//     the statement's first MFMA and what hipcc places in front of it that 32 s_nops narrowed but did not close: the builtin stays.)
// The softmax arithmetic is attn_fwd_kernel's (running maximum per tile, scores scaled inside the exp2's fma): the same values up to the order of the fp32 sums.
// =====================================================================================================
__global__ __launch_bounds__(256) void attn_fwd_d256_kernel(AttnArgs A)
{
    constexpr int D = 256, kRow = D * 2, kTile = 64 * kRow, PPW = 8;      // bytes of a row / of a 64-key tile; 1 KiB pieces per wave and operand and tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // 2 x (K, V) tiles, the row's key mask, 64 tile flags
    float *lds_maskrow = reinterpret_cast<float *>(smem + 4 * kTile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
    int qblk, head_in, group;
    map_block((int)blockIdx.x, (A.S + 127) / 128, A.Hq / A.Hkv, A.B * A.Hkv, true, qblk, head_in, group);
    const int b = group / A.Hkv, g = group % A.Hkv, hq = g * (A.Hq / A.Hkv) + head_in;
    const int q0 = qblk * 128, qw0 = q0 + wave * 32;
    const int qi = qw0 + lr;
    const bool qvalid = qi < A.S;
    const long long rowbase = (long long)b * A.S;
    const unsigned short *Q = A.q + (long long)hq * D, *K = A.k + (long long)g * D, *V = A.v + (long long)g * D;
    const int k_end = min(A.S, q0 + 128);
    const int wave_qmax = qw0 + 31;
    const int last_tile = (k_end - 1) / 64;
    const int tail_rows = A.S - last_tile * 64;                           // rows of the last tile that exist (64: whole)
    // piece i of this wave: tile rows (wave * 8 + i) * 2 + (lane >> 5), the lane's 16-byte slot lane & 31 of the LDS row takes global chunk slot ^ swizzle(row)
    unsigned offK[PPW], offV[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave * PPW + i) * 2 + (lane >> 5), slot = lane & 31;
        offK[i] = (unsigned)(((long long)r * A.ldk + (slot ^ (r & 15)) * 8) * 2);
        offV[i] = (unsigned)(((long long)r * A.ldv + (slot ^ ((r & 7) << 2)) * 8) * 2);
    }
    const unsigned char *kb_next = reinterpret_cast<const unsigned char *>(K + rowbase * A.ldk), *vb_next = reinterpret_cast<const unsigned char *>(V + rowbase * A.ldv);
    const long long stepK = 128ll * A.ldk, stepV = 128ll * A.ldv;
    int t_next = 0;
    unsigned slot_next = 0;
    // piece i of the next tile's K and of its V image (round 6: a K piece behind each group of the score products, a V piece behind each group of the P.V products -- issued together at the top of the trip the sixteen pieces
    // held the wave for ~1 000 cycles with the matrix pipe idle; behind a group they run under its four MFMAs)
    auto issue_piece = [&](int which, int i) __attribute__((always_inline)) {      // which: 0 the K image, 1 the V image
        unsigned off = which ? offV[i] : offK[i];
        if (t_next == last_tile && tail_rows < 64) {                      // (uniform, once per workgroup at most) rows past the last key re-read it: masked as keys >= S
            const int r = (wave * PPW + i) * 2 + (lane >> 5), slot = lane & 31, rt = min(r, tail_rows - 1);
            off = which ? (unsigned)(((long long)rt * A.ldv + (slot ^ ((r & 7) << 2)) * 8) * 2) : (unsigned)(((long long)rt * A.ldk + (slot ^ (r & 15)) * 8) * 2);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((which ? vb_next : kb_next) + off),
                                         (__attribute__((address_space(3))) void *)(smem + slot_next + which * kTile + (wave * PPW + i) * 1024), 16, 0, 0);
    };
    auto advance_next = [&]() { if (t_next < last_tile) { ++t_next; kb_next += stepK; vb_next += stepV; } slot_next ^= 2 * kTile; };
    auto issue_next = [&]() {                                             // UNCONDITIONAL (past the last tile the last one is issued again)
        if (t_next == last_tile && tail_rows < 64) {                      // (uniform, once per workgroup at most) rows past the last key re-read it: masked as keys >= S
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                const int r = (wave * PPW + i) * 2 + (lane >> 5), slot = lane & 31, rt = min(r, tail_rows - 1);
                const unsigned ok = (unsigned)(((long long)rt * A.ldk + (slot ^ (r & 15)) * 8) * 2), ov = (unsigned)(((long long)rt * A.ldv + (slot ^ ((r & 7) << 2)) * 8) * 2);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb_next + ok),
                                                 (__attribute__((address_space(3))) void *)(smem + slot_next + (wave * PPW + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb_next + ov),
                                                 (__attribute__((address_space(3))) void *)(smem + slot_next + kTile + (wave * PPW + i) * 1024), 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kb_next + offK[i]),
                                                 (__attribute__((address_space(3))) void *)(smem + slot_next + (wave * PPW + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vb_next + offV[i]),
                                                 (__attribute__((address_space(3))) void *)(smem + slot_next + kTile + (wave * PPW + i) * 1024), 16, 0, 0);
            }
        }
        if (t_next < last_tile) { ++t_next; kb_next += stepK; vb_next += stepV; }
        slot_next ^= 2 * kTile;
    };
    issue_next();
    bf16x8 qf[D / 16];
    load_row_frags<D>(qf, Q, A.ldq, rowbase + qi, qvalid, h);
    lean_fill_mask<4>(lds_maskrow, A.mask + rowbase, A.S, (k_end + 63) & ~63);
    f32x16 accO[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db) accO[db] = splat16(0.f);
    float m = -INFINITY, l = 0.f;
    const float sc = A.scale * kLog2e;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // tile 0 and Q
    __syncthreads();
    const unsigned long long padbits = lean_pad_bits(lds_maskrow, (k_end + 63) & ~63);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    // this lane's K row fragment (key lr, k-step 0) inside a K image: k-step ks is the address ^ (ks << 5), key 32 + lr 16 KiB further (the swizzle repeats every 16 rows)
    const unsigned kbase = lr * kRow + ((h ^ (lr & 15)) << 4);      // (an offset: the XORs below must not see the LDS base)
    // this lane's first transposing read inside a V image for d block 0: block db is the address ^ (db << 6), the second read 8 keys = 4 KiB further, the (kb, s2) row groups go
    // into the offset field
    unsigned vbase;
    {
        const int a = lr >> 4, q = (lr & 15) >> 2, p = lr & 3;
        const int key = 4 * h + q;
        vbase = key * kRow + ((((key & 7) << 2) | (2 * a + (p >> 1))) << 4) + (p & 1) * 8;
    }
    unsigned img = 0;                                                     // byte offset of the current tile's ring slot
    for (int k0 = 0, it = 0; k0 < k_end; k0 += 64, ++it) {
        const float *lds_mask = lds_maskrow + k0;                         // (tile it + 1 goes into the other slot: its readers passed the barrier that ended the previous trip)
        if (k0 > wave_qmax) issue_next();
        if (k0 <= wave_qmax) {
            const bool need_mask = (k0 + 63 > qw0) || lean_tile_padded(padbits, it);
            f32x16 sacc[2] = {splat16(0.f), splat16(0.f)};
#pragma unroll
            for (int ks = 0; ks < D / 16; ks += 2) {                      // eight batches of four fragments (two k-steps x two key halves) and their four products
                bf16x8 f00, f01, f10, f11;
                lds_frags2x2_wait<0, 32 * kRow>(f00, f01, f10, f11, (kbase ^ (unsigned)(ks << 5)) + img + lds0, (kbase ^ (unsigned)((ks + 1) << 5)) + img + lds0);
                sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f00, qf[ks], sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f01, qf[ks], sacc[1], 0, 0, 0);
                sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f10, qf[ks + 1], sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f11, qf[ks + 1], sacc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                issue_piece(0, ks / 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            float p[2][16];
            float tmax = -INFINITY;
            if (need_mask) {                                              // (uniform) the tile touches this wave's diagonal or holds padded keys
                f4v mv[2][4];
                const unsigned ma = (unsigned)(size_t)(__attribute__((address_space(3))) float *)const_cast<float *>(lds_mask) + 16 * h;
                lds_rows4_wait<0>(mv[0], ma);
                lds_rows4_wait<128>(mv[1], ma);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // key inside the tile
                        const bool vis = (k0 + kl <= qi) & (mv[kb][r >> 2][r & 3] != 0.f);
                        const float v = vis ? sacc[kb][r] : -INFINITY;
                        p[kb][r] = v;
                        tmax = fmaxf(tmax, v);
                    }
            } else {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { p[kb][r] = sacc[kb][r]; tmax = fmaxf(tmax, sacc[kb][r]); }
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * sc;            // p holds raw scores; sc > 0, so the maximum scales with them
            const float m_new = fmaxf(m, tmax);
            const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;      // no key visible yet: every p below is exp2(-inf) = 0
            const float alpha = fast_exp2(m - m_safe);                    // m = -inf -> 0 (accumulators are still zero then)
            float lsum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float e = fast_exp2(__builtin_fmaf(p[kb][r], sc, -m_safe)); p[kb][r] = e; lsum += e; }
            l = l * alpha + lsum;
            m = m_new;
            if (__any(alpha != 1.f)) {                                    // once the running maxima have settled the accumulators need no rescale
#pragma unroll
                for (int db = 0; db < D / 32; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) accO[db][r] *= alpha;
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const bf16x8 pf0 = frag_from_acc(&p[kb][0]), pf1 = frag_from_acc(&p[kb][8]);
#pragma unroll
                for (int dp = 0; dp < D / 64; ++dp) {                     // pairs of d blocks: four transposed fragments (two k-steps x two blocks) and their four products
                    bf16x8 vfr[2][2];
                    const unsigned a0 = (vbase ^ (unsigned)((2 * dp) << 6)) + img + lds0 + kTile, a1 = (vbase ^ (unsigned)((2 * dp + 1) << 6)) + img + lds0 + kTile;
                    if (kb == 0) tr_frags4_wait<0, 16 * kRow>(vfr, a0, a0 + 8 * kRow, a1, a1 + 8 * kRow);
                    else tr_frags4_wait<32 * kRow, 48 * kRow>(vfr, a0, a0 + 8 * kRow, a1, a1 + 8 * kRow);
                    accO[2 * dp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0][0], pf0, accO[2 * dp], 0, 0, 0);
                    accO[2 * dp + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0][1], pf0, accO[2 * dp + 1], 0, 0, 0);
                    accO[2 * dp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[1][0], pf1, accO[2 * dp], 0, 0, 0);
                    accO[2 * dp + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[1][1], pf1, accO[2 * dp + 1], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    issue_piece(1, kb * 4 + dp);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            advance_next();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // this wave's pieces of tile it + 1 have landed
        __builtin_amdgcn_s_barrier();                                     // ... and everybody else's; all reads of tile it are done
        img ^= 2 * kTile;
    }
    const float lt = l + __shfl_xor(l, 32, 64);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    store_accT<D / 32>(accO, A.o + (long long)hq * D, A.ldo, rowbase + qi, qvalid, h, inv);
    if (qvalid && h == 0) A.lse[((long long)b * A.Hq + hq) * A.S + qi] = lt > 0.f ? m + log2f(lt) : INFINITY;
}

// head_dim 256 dQ: attention_d256.hip (round 6; round 4's LDS-DMA kernel with asm reads is in the history).  The swizzle its images and the dK / dV kernel's share: 16-byte
// chunk c of row r lies at c ^ f(r), f(r) = (r & 3) << 2 | (r >> 2) & 3 (attention_common.inc) -- sixteen consecutive rows put one chunk on sixteen different bank groups, and
// the eight key rows of a transposing read put one 64-byte group on all four 64-byte positions of the bank cycle, twice each.

// head_dim 256 dK / dV pair kernel: attention_d256.hip (round 6; round 4's form with asm reads is in the history).

struct LeanGeom { int hw_log2; unsigned grid; };
LeanGeom lean_geom(int seq, int n_q_heads, int n_kv_heads, int batch)
{
    const int G = n_q_heads / n_kv_heads;
    int l2 = 0;
    while ((2 << l2) <= g_lean_waves && G % (2 << l2) == 0) ++l2;
    const int rows = (g_lean_waves >> l2) * 32;
    return {l2, (unsigned)((seq + rows - 1) / rows) * (unsigned)(n_q_heads >> l2) * (unsigned)batch};
}

// ---- dynamic LDS of each kernel family, in bytes (mask_lds_bytes, ring256_lds_bytes: attention_common.inc; the head_dim-256 backward: attention_d256.hip) ----
// register-staged (attn_fwd_kernel<D>, attn_bwd_dq_kernel<D>, attn_bwd_dkv_kernel<D> / attn_bwd_dkv_pair_kernel<D>): tile buffers + the row's key mask / + the statistics
long long fwd_lds_bytes(int D, int seq) { return 4 * 128 * D + mask_lds_bytes(seq); }
long long dq_lds_bytes(int D, int seq) { return 3 * 128 * D + mask_lds_bytes(seq); }
int dkv_lds_bytes(int D) { return 4 * 128 * D + 512; }
// round-2 LDS-DMA, head_dim 64 (attn_fwd_kernel<64, true>, attn_bwd_dq_dma_kernel; attn_bwd_dkv_dma_kernel): rings of three
long long dma_lds_bytes(int seq) { return 6 * 128 * 64 + mask_lds_bytes(seq); }
int dkv_dma_lds_bytes() { return 3 * (2 * 128 * 64 + 1024); }
// lean, head_dim 64 (attn_fwd_lean_kernel, attn_bwd_dq_lean_kernel: K / V ring, the key mask, 64 tile flags; attn_bwd_dkv_lean_kernel: Q / dO ring + a wave's statistics)
long long lean_lds_bytes(int seq) { return 2 * kLeanRing * 128 * 64 + mask_lds_bytes(seq) + 256; }
int dkv_lean_lds_bytes(int waves) { return kLeanRing * (2 * 128 * 64 + waves * 256); }
// the most any form of the head dim that check_args() lets through may ask for at this length: the lean kernels at 64 (with their tile flags: every staging mode
// takes the same lengths), the register-staged forward otherwise (the head_dim-256 ring is used only where it fits: plan_fwd / plan_bwd)
long long attn_lds_max(int D, int seq) { return D == 64 ? std::max(lean_lds_bytes(seq), fwd_lds_bytes(D, seq)) : fwd_lds_bytes(D, seq); }

// head_dim 256: may this pair of operands be staged by LDS-DMA?  16-byte aligned rows, and 64 rows + a row of 512 bytes inside the 32-bit per-lane offsets
bool dma256_ok(const void *a, long long ld_a, const void *b, long long ld_b)
{
    return (ld_a & 7) == 0 && (ld_b & 7) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && 64 * ld_a * 2 + 512 <= 0xFFFFFFFFll && 64 * ld_b * 2 + 512 <= 0xFFFFFFFFll;
}

int refuse(const char *who, const char *what, int code)
{
    ecgb::set_error(std::string(who) + ": " + what);
    return code;
}

int check_args(const AttnArgs &A, int D, const char *who)
{
    if (A.B <= 0 || A.S <= 0 || A.Hq <= 0 || A.Hkv <= 0 || A.Hq % A.Hkv) return refuse(who, "bad shape", ECGB_ERR_INVALID);
    if (D != 64 && D != 128 && D != 256) return refuse(who, "head_dim must be 64, 128 or 256", ECGB_ERR_UNSUPPORTED);
    if (A.ldq % 8 || A.ldk % 8 || A.ldv % 8 || A.ldo % 8) return refuse(who, "row strides must be multiples of 8 elements", ECGB_ERR_UNSUPPORTED);
    if (attn_lds_max(D, A.S) > kLdsMax)
        return refuse(who, "sequence too long for the key mask in LDS (head_dim 256: 8 192 keys, 128: 24 576, 64: 28 608)", ECGB_ERR_UNSUPPORTED);
    return ECGB_OK;
}
// the entry points' first check
int check_ptrs(const char *who, std::initializer_list<const void *> required)
{
    for (const void *p : required)
        if (!p) return refuse(who, "null pointer", ECGB_ERR_INVALID);
    return ECGB_OK;
}
// what ecgb_attn_fwd_dropout / ecgb_attn_bwd_dropout ask of (p, head_dim); p == 0 is the plain call
int check_drop(float p, int head_dim, const char *who)
{
    if (!(p >= 0.f && p < 1.f)) return refuse(who, "0 <= p < 1 required", ECGB_ERR_INVALID);
    if (p > 0.f && head_dim != 64) return refuse(who, "dropout on the probabilities is built for head_dim 64 only", ECGB_ERR_UNSUPPORTED);
    return ECGB_OK;
}
// what ecgb_attn_bwd_rope asks: store_accT_rope_inv is in the lean backward kernels only and stores 16 bytes at a time
int check_rope(const void *dq, long long lddq, const void *dk, long long lddk, const void *rope_cos, const void *rope_sin, int head_dim, const char *who)
{
    if (!rope_cos || !rope_sin) return refuse(who, "NULL table", ECGB_ERR_INVALID);
    if (head_dim != 64 || (g_attn_dma & 0x703) != 2 || (lddq & 7) || (lddk & 7) || (((uintptr_t)dq | (uintptr_t)dk | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15))
        return refuse(who, "head_dim 64 on the lean kernels with 16-byte aligned gradient rows only", ECGB_ERR_UNSUPPORTED);
    return ECGB_OK;
}

// ---- the argument block: the forward's fields, what the backward adds, dropout, what a plan decides ----
AttnArgs attn_args(const void *q, long long ldq, const void *k, long long ldk, const void *v, long long ldv, const float *mask, const void *o, long long ldo,
                   const float *lse, int batch, int seq, int n_q_heads, int n_kv_heads, float scale)
{
    AttnArgs A = {};
    A.q = (const unsigned short *)q; A.k = (const unsigned short *)k; A.v = (const unsigned short *)v;
    A.ldq = ldq; A.ldk = ldk; A.ldv = ldv; A.mask = mask; A.o = (unsigned short *)const_cast<void *>(o); A.ldo = ldo; A.lse = const_cast<float *>(lse);
    A.B = batch; A.S = seq; A.Hq = n_q_heads; A.Hkv = n_kv_heads; A.scale = scale;
    return A;
}
void attn_args_bwd(AttnArgs &A, const void *d_o, float *delta, void *dq, long long lddq, void *dk, long long lddk, void *dv, long long lddv, void *scratch,
                   const float *rope_cos, const float *rope_sin)
{
    A.d_o = (const unsigned short *)d_o; A.delta = delta;
    A.dq = (unsigned short *)dq; A.dk = (unsigned short *)dk; A.dv = (unsigned short *)dv;
    A.lddq = lddq; A.lddk = lddk; A.lddv = lddv;
    A.slab = (float *)scratch;
    A.rope_cos = rope_cos; A.rope_sin = rope_sin;
}
void set_drop(AttnArgs &A, float p, uint64_t seed)
{
    A.drop_seed = (unsigned long long)seed;
    A.drop_thr = drop_threshold(p);
    A.drop_inv = 1.0f / (1.0f - p);                          // (as ecgb_dropout_bf16 forms it)
}

// ---- the dispatch: which kernels a call launches, in order, and what it sets in the argument block.  No HIP call: ecgb_attn_launch_plan reads it without a device ----
struct AttnPlan {
    AttnLaunch launch[4];
    int n = 0;
    int lean_hw_log2 = 0, head_splits = 0;
    unsigned short *pbuf = nullptr;
    void add(const AttnLaunch &l) { launch[n++] = l; }
    void add(AttnKern kern, const char *name, unsigned grid, unsigned block, long long lds) { launch[n++] = {kern, name, grid, block, (int)lds}; }
};
void set_plan(AttnArgs &A, const AttnPlan &P) { A.lean_hw_log2 = P.lean_hw_log2; A.head_splits = P.head_splits; A.pbuf = P.pbuf; }

// head_dim 256 with few (batch, KV head, key block) workgroups: the causal key blocks differ 16-fold in work and one launch of <= 256
// workgroups takes as long as its heaviest one (key block 0).  Splitting a group's query heads over 2..4 workgroups gives the scheduler
// pieces to balance with (heaviest first); the price is fp32 partial slabs and a small ordered reduction.
int dkv_head_splits(int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim)
{
    if (head_dim != 256) return 1;
    const int G = n_q_heads / n_kv_heads;
    const long long wgs = (long long)((seq + 127) / 128) * n_kv_heads * batch * 2;
    int hs = 1;
    while (wgs * hs < 1024 && hs * 2 <= 4 && G % (hs * 2) == 0) hs *= 2;
    return hs;
}
size_t dkv_slab_bytes(int hs, int batch, int seq, int n_kv_heads, int head_dim)
{
    return hs > 1 ? (size_t)2 * hs * batch * seq * n_kv_heads * head_dim * sizeof(float) : 0;
}
// head_dim 256 (round 6): room for the probabilities the dK pass hands to the dV kernel (AttnArgs::pbuf), bf16 over whole 128-key x 64-query tiles
size_t attn_bwd_p_bytes(int batch, int seq, int n_q_heads, int head_dim)
{
    if (head_dim != 256 || !g_attn_d256_pass_p) return 0;
    return (size_t)batch * n_q_heads * ((seq + 127) / 128) * ((seq + 63) / 64) * (128 * 64 * 2);
}

// head_dim 64 by ecgb_set_attn_fwd_staging (the lean kernels, | 0x100: the round-2 LDS-DMA kernel, 0: register-staged) -- with dropout always register-staged;
// head_dim 256: LDS-DMA staging (round 4) where its ring fits the CU's LDS and dma256_ok(k, v), mode 0 keeps the register-staged kernel (A/B, tests)
int plan_fwd(const AttnArgs &A, int D, bool drop, const char *who, AttnPlan &P)
{
    const int rc = check_args(A, D, who);
    if (rc) return rc;
    const int seq = A.S, mode = drop ? 0 : g_attn_dma & 3;
    const unsigned grid = (unsigned)((seq + 127) / 128) * (unsigned)A.Hq * (unsigned)A.B;       // 1-D: map_block() deals blocks to XCDs
    if (D == 64 && mode == 2 && !(g_attn_dma & 0x100)) {
        const LeanGeom lg = lean_geom(seq, A.Hq, A.Hkv, A.B);
        P.lean_hw_log2 = lg.hw_log2;
        P.add(g_lean_waves == 8 ? attn_fwd_lean_kernel<8> : attn_fwd_lean_kernel<4>, "attn_fwd_lean_kernel", lg.grid, g_lean_waves * 64, lean_lds_bytes(seq));
    } else if (D == 64 && mode) {
        P.add(attn_fwd_kernel<64, true>, "attn_fwd_kernel<64, dma>", grid, 256, dma_lds_bytes(seq));
    } else if (D == 64 && !drop) {
        P.add(attn_fwd_kernel<64>, "attn_fwd_kernel<64>", grid, 256, fwd_lds_bytes(64, seq));
    } else if (D == 128) {
        P.add(attn_fwd_kernel<128>, "attn_fwd_kernel<128>", grid, 256, fwd_lds_bytes(128, seq));
    } else if (D == 256 && mode && ring256_lds_bytes(seq) <= kLdsMax && dma256_ok(A.k, A.ldk, A.v, A.ldv)) {
        P.add(attn_fwd_d256_kernel, "attn_fwd_d256_kernel", grid, 256, ring256_lds_bytes(seq));
    } else if (D == 256) {
        P.add(attn_fwd_kernel<256>, "attn_fwd_kernel<256>", grid, 256, fwd_lds_bytes(256, seq));
    } else {                                                                                    // dropout (head_dim 64: check_drop)
        P.add(attn_fwd_kernel<64, false, true>, "attn_fwd_kernel<64, dropout>", grid, 256, fwd_lds_bytes(64, seq));
    }
    return ECGB_OK;
}

// dQ, then dK / dV (head_dim 256: the pair kernel, or with the whole of ecgb_attn_bwd_scratch_bytes() the dK pass that hands its probabilities to a dV kernel), then
// the reduction of the head-split slabs.  head_dim 64: | 0x200 / 0x400 keep dQ / dK-dV alone on the round-2 kernels; with dropout the register-staged DROP forms
int plan_bwd(const AttnArgs &A, int D, bool drop, const void *scratch, size_t scratch_bytes, const char *who, AttnPlan &P)
{
    const int rc = check_args(A, D, who);
    if (rc) return rc;
    if (A.lddq % 4 || A.lddk % 4 || A.lddv % 4) return refuse(who, "gradient row strides must be multiples of 4", ECGB_ERR_UNSUPPORTED);
    const int seq = A.S, mode = drop ? 0 : g_attn_dma & 3;
    P.head_splits = dkv_head_splits(A.B, seq, A.Hq, A.Hkv, D);
    const unsigned hs = (unsigned)P.head_splits;
    const size_t slab_bytes = dkv_slab_bytes(P.head_splits, A.B, seq, A.Hkv, D);
    const bool scratch_ok = scratch && ((uintptr_t)scratch & 15) == 0;
    if (hs > 1 && (!scratch_ok || scratch_bytes < slab_bytes))
        return refuse(who, "scratch for the partial dK / dV slabs (16-byte aligned; ecgb_attn_bwd_scratch_bytes() says how much) required for this shape", ECGB_ERR_INVALID);
    const unsigned nblk = (unsigned)((seq + 127) / 128);
    const unsigned gq = nblk * (unsigned)A.Hq * (unsigned)A.B, gk = nblk * (unsigned)A.Hkv * (unsigned)A.B;       // 1-D: map_block() deals blocks to XCDs
    if (D == 64 && !drop) {
        const bool lq_lean = mode == 2 && !(g_attn_dma & 0x200), lk_lean = mode == 2 && !(g_attn_dma & 0x400);
        const LeanGeom lg = lean_geom(seq, A.Hq, A.Hkv, A.B);
        if (mode) P.lean_hw_log2 = lg.hw_log2;
        if (lq_lean) P.add(g_lean_waves == 8 ? attn_bwd_dq_lean_kernel<8> : attn_bwd_dq_lean_kernel<4>, "attn_bwd_dq_lean_kernel", lg.grid, g_lean_waves * 64, lean_lds_bytes(seq));
        else if (mode) P.add(attn_bwd_dq_dma_kernel, "attn_bwd_dq_dma_kernel", gq, 256, dma_lds_bytes(seq));
        else P.add(attn_bwd_dq_kernel<64>, "attn_bwd_dq_kernel<64>", gq, 256, dq_lds_bytes(64, seq));
        const unsigned gkl = (unsigned)(((seq + g_lean_waves * 32 - 1) / (g_lean_waves * 32) + 1) / 2) * (unsigned)A.Hkv * (unsigned)A.B;   // key blocks in pairs (j, n - 1 - j)
        if (lk_lean) P.add(g_lean_waves == 8 ? attn_bwd_dkv_lean_kernel<8> : attn_bwd_dkv_lean_kernel<4>, "attn_bwd_dkv_lean_kernel", gkl, g_lean_waves * 64, dkv_lean_lds_bytes(g_lean_waves));
        else if (mode) P.add(attn_bwd_dkv_dma_kernel, "attn_bwd_dkv_dma_kernel", gk, 256, dkv_dma_lds_bytes());
        else P.add(attn_bwd_dkv_kernel<64, 1, 0>, "attn_bwd_dkv_kernel<64>", gk, 256, dkv_lds_bytes(64));
    } else if (D == 128) {
        P.add(attn_bwd_dq_kernel<128>, "attn_bwd_dq_kernel<128>", gq, 256, dq_lds_bytes(128, seq));
        P.add(attn_bwd_dkv_kernel<128, 1, 0>, "attn_bwd_dkv_kernel<128>", gk, 256, dkv_lds_bytes(128));
    } else if (D == 256) {
        if (mode && ring256_lds_bytes(seq) <= kLdsMax && dma256_ok(A.k, A.ldk, A.v, A.ldv)) P.add(ecgb_attn::bwd_dq_d256(gq, seq));
        else P.add(attn_bwd_dq_kernel<256>, "attn_bwd_dq_kernel<256>", gq, 256, dq_lds_bytes(256, seq));
        const size_t p_bytes = attn_bwd_p_bytes(A.B, seq, A.Hq, D);
        if (!(mode && dma256_ok(A.q, A.ldq, A.d_o, A.ldo))) {
            P.add(attn_bwd_dkv_pair_kernel<256>, "attn_bwd_dkv_pair_kernel<256>", gk * 2 * hs, 256, dkv_lds_bytes(256));
        } else if (p_bytes > 0 && scratch_ok && scratch_bytes >= slab_bytes + p_bytes) {
            P.pbuf = reinterpret_cast<unsigned short *>(reinterpret_cast<unsigned char *>(const_cast<void *>(scratch)) + slab_bytes);
            P.add(ecgb_attn::bwd_dk_d256(gk * hs));
            P.add(ecgb_attn::bwd_dv_d256(gk * hs));
        } else {
            P.add(ecgb_attn::bwd_dkv_pair_d256(gk * 2 * hs));
        }
        if (hs > 1) P.add(attn_dkv_reduce_kernel<256>, "attn_dkv_reduce_kernel<256>", 2048, 256, 0);
    } else {                                                                                    // dropout (head_dim 64: check_drop)
        P.add(attn_bwd_dq_kernel<64, true>, "attn_bwd_dq_kernel<64, dropout>", gq, 256, dq_lds_bytes(64, seq));
        P.add(attn_bwd_dkv_kernel<64, 1, 0, true>, "attn_bwd_dkv_kernel<64, dropout>", gk, 256, dkv_lds_bytes(64));
    }
    return ECGB_OK;
}

int run_plan(AttnArgs &A, const AttnPlan &P, void *stream)
{
    set_plan(A, P);
    for (int i = 0; i < P.n; ++i) {
        const AttnLaunch &l = P.launch[i];
        const int rc = launch_attn(l.kern, l.name, l.grid, l.block, l.lds, stream, A);
        if (rc) return rc;
    }
    return ECGB_OK;
}

// the one forward body and the one backward body; p > 0: dropout on the probabilities from (p, seed)
int attn_fwd_impl(const char *who, const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                  const float *attn_mask_dev, void *o_dev, long long ldo, float *lse_dev, int batch, int seq,
                  int n_q_heads, int n_kv_heads, int head_dim, float scale, float p, uint64_t seed, void *stream)
{
    AttnArgs A = attn_args(q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, ldo, lse_dev, batch, seq, n_q_heads, n_kv_heads, scale);
    if (p > 0.f) set_drop(A, p, seed);
    AttnPlan P;
    const int rc = plan_fwd(A, head_dim, p > 0.f, who, P);
    return rc ? rc : run_plan(A, P, stream);
}
int attn_bwd_impl(const char *who, const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                  const float *attn_mask_dev, const void *o_dev, const void *do_dev, long long ldo,
                  const float *lse_dev, float *delta_dev, void *dq_dev, long long lddq, void *dk_dev, long long lddk,
                  void *dv_dev, long long lddv, int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                  float scale, void *scratch_dev, size_t scratch_bytes, void *stream, const float *rope_cos, const float *rope_sin, float p, uint64_t seed)
{
    AttnArgs A = attn_args(q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, ldo, lse_dev, batch, seq, n_q_heads, n_kv_heads, scale);
    attn_args_bwd(A, do_dev, delta_dev, dq_dev, lddq, dk_dev, lddk, dv_dev, lddv, scratch_dev, rope_cos, rope_sin);
    if (p > 0.f) set_drop(A, p, seed);
    AttnPlan P;
    const int rc = plan_bwd(A, head_dim, p > 0.f, scratch_dev, scratch_bytes, who, P);
    return rc ? rc : run_plan(A, P, stream);
}

}  // namespace

extern "C" int ecgb_attn_fwd(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                             const float *attn_mask_dev, void *o_dev, long long ldo, float *lse_dev, int batch, int seq,
                             int n_q_heads, int n_kv_heads, int head_dim, float scale, void *stream)
{
    const char *who = "ecgb_attn_fwd";
    if (int rc = check_ptrs(who, {q_dev, k_dev, v_dev, attn_mask_dev, o_dev, lse_dev})) return rc;
    return attn_fwd_impl(who, q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, ldo, lse_dev, batch, seq, n_q_heads, n_kv_heads, head_dim, scale, 0.f, 0, stream);
}

extern "C" int ecgb_attn_fwd_dropout(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                                     const float *attn_mask_dev, void *o_dev, long long ldo, float *lse_dev, int batch, int seq,
                                     int n_q_heads, int n_kv_heads, int head_dim, float scale, float p, uint64_t seed, void *stream)
{
    const char *who = "ecgb_attn_fwd_dropout";
    if (int rc = check_ptrs(who, {q_dev, k_dev, v_dev, attn_mask_dev, o_dev, lse_dev})) return rc;
    if (int rc = check_drop(p, head_dim, who)) return rc;
    return attn_fwd_impl(who, q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, ldo, lse_dev, batch, seq, n_q_heads, n_kv_heads, head_dim, scale, p, seed, stream);
}

extern "C" size_t ecgb_attn_bwd_scratch_bytes(int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim)
{
    if (batch <= 0 || seq <= 0 || n_q_heads <= 0 || n_kv_heads <= 0 || n_q_heads % n_kv_heads) return 0;
    const int hs = dkv_head_splits(batch, seq, n_q_heads, n_kv_heads, head_dim);
    return dkv_slab_bytes(hs, batch, seq, n_kv_heads, head_dim) + attn_bwd_p_bytes(batch, seq, n_q_heads, head_dim);
}

extern "C" int ecgb_attn_bwd(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                             const float *attn_mask_dev, const void *o_dev, const void *do_dev, long long ldo,
                             const float *lse_dev, float *delta_dev, void *dq_dev, long long lddq, void *dk_dev, long long lddk,
                             void *dv_dev, long long lddv, int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                             float scale, void *scratch_dev, size_t scratch_bytes, void *stream)
{
    const char *who = "ecgb_attn_bwd";
    if (int rc = check_ptrs(who, {q_dev, k_dev, v_dev, attn_mask_dev, o_dev, lse_dev, do_dev, delta_dev, dq_dev, dk_dev, dv_dev})) return rc;
    return attn_bwd_impl(who, q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, do_dev, ldo, lse_dev, delta_dev, dq_dev, lddq, dk_dev, lddk, dv_dev, lddv,
                         batch, seq, n_q_heads, n_kv_heads, head_dim, scale, scratch_dev, scratch_bytes, stream, nullptr, nullptr, 0.f, 0);
}

// the backward of ecgb_attn_fwd_dropout (o_dev and lse_dev are that forward's): two launches of the register-staged kernels' DROP forms; the scratch is not used
extern "C" int ecgb_attn_bwd_dropout(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                                     const float *attn_mask_dev, const void *o_dev, const void *do_dev, long long ldo,
                                     const float *lse_dev, float *delta_dev, void *dq_dev, long long lddq, void *dk_dev, long long lddk,
                                     void *dv_dev, long long lddv, int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                     float scale, void *scratch_dev, size_t scratch_bytes, float p, uint64_t seed, void *stream)
{
    const char *who = "ecgb_attn_bwd_dropout";
    if (int rc = check_ptrs(who, {q_dev, k_dev, v_dev, attn_mask_dev, o_dev, lse_dev, do_dev, delta_dev, dq_dev, dk_dev, dv_dev})) return rc;
    if (int rc = check_drop(p, head_dim, who)) return rc;
    return attn_bwd_impl(who, q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, do_dev, ldo, lse_dev, delta_dev, dq_dev, lddq, dk_dev, lddk, dv_dev, lddv,
                         batch, seq, n_q_heads, n_kv_heads, head_dim, scale, scratch_dev, scratch_bytes, stream, nullptr, nullptr, p, seed);
}

// ecgb_attn_bwd followed by RoPE's backward on dQ and dK (ecgb_rope, inverse), in the attention kernels' own stores: q and k are the ROTATED projections the forward
// saw, dq / dk come out as gradients of the unrotated ones.  rope_cos_dev / rope_sin_dev: [batch * seq, 32] fp32, the tables ecgb_rope takes.  head_dim 64 on the
// lean kernels with 16-byte aligned dq / dk rows only: ECGB_ERR_UNSUPPORTED otherwise, and the caller runs the two steps apart (the same bits either way).
extern "C" int ecgb_attn_bwd_rope(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const void *v_dev, long long ldv,
                                  const float *attn_mask_dev, const void *o_dev, const void *do_dev, long long ldo,
                                  const float *lse_dev, float *delta_dev, void *dq_dev, long long lddq, void *dk_dev, long long lddk,
                                  void *dv_dev, long long lddv, const float *rope_cos_dev, const float *rope_sin_dev, int batch, int seq, int n_q_heads,
                                  int n_kv_heads, int head_dim, float scale, void *scratch_dev, size_t scratch_bytes, void *stream)
{
    const char *who = "ecgb_attn_bwd_rope";
    if (int rc = check_ptrs(who, {q_dev, k_dev, v_dev, attn_mask_dev, o_dev, lse_dev, do_dev, delta_dev, dq_dev, dk_dev, dv_dev})) return rc;
    if (int rc = check_rope(dq_dev, lddq, dk_dev, lddk, rope_cos_dev, rope_sin_dev, head_dim, who)) return rc;
    return attn_bwd_impl(who, q_dev, ldq, k_dev, ldk, v_dev, ldv, attn_mask_dev, o_dev, do_dev, ldo, lse_dev, delta_dev, dq_dev, lddq, dk_dev, lddk, dv_dev, lddv,
                         batch, seq, n_q_heads, n_kv_heads, head_dim, scale, scratch_dev, scratch_bytes, stream, rope_cos_dev, rope_sin_dev, 0.f, 0);
}

// The plan of a call, for reading without a device: what `entry` (0 ecgb_attn_fwd, 1 ecgb_attn_bwd, 2 ecgb_attn_bwd_rope, 3 ecgb_attn_fwd_dropout, 4 ecgb_attn_bwd_dropout) would
// launch for these operands under the current switches.  The addresses count for their alignment only; mask, o, lse and delta are taken as given.
extern "C" int ecgb_attn_launch_plan(int entry, float p, const void *q, long long ldq, const void *k, long long ldk, const void *v, long long ldv, const void *d_o, long long ldo,
                                     const void *dq, long long lddq, const void *dk, long long lddk, const void *dv, long long lddv, const void *rope_cos, const void *rope_sin,
                                     int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim, const void *scratch, size_t scratch_bytes,
                                     int *n_launches, int *grid_block_lds, long long *args_set, char *names, int names_cap)
{
    static const char *const kWho[] = {"ecgb_attn_fwd", "ecgb_attn_bwd", "ecgb_attn_bwd_rope", "ecgb_attn_fwd_dropout", "ecgb_attn_bwd_dropout"};
    if (entry < 0 || entry > 4 || !n_launches || !grid_block_lds || !args_set || !names || names_cap <= 0) return refuse("ecgb_attn_launch_plan", "bad arguments", ECGB_ERR_INVALID);
    const char *who = kWho[entry];
    const bool fwd = entry == 0 || entry == 3, drop_entry = entry >= 3;
    if (int rc = fwd ? check_ptrs(who, {q, k, v}) : check_ptrs(who, {q, k, v, d_o, dq, dk, dv})) return rc;
    if (drop_entry) { if (int rc = check_drop(p, head_dim, who)) return rc; }
    if (entry == 2) { if (int rc = check_rope(dq, lddq, dk, lddk, rope_cos, rope_sin, head_dim, who)) return rc; }
    AttnArgs A = attn_args(q, ldq, k, ldk, v, ldv, nullptr, nullptr, ldo, nullptr, batch, seq, n_q_heads, n_kv_heads, 1.f);
    if (!fwd) attn_args_bwd(A, d_o, nullptr, const_cast<void *>(dq), lddq, const_cast<void *>(dk), lddk, const_cast<void *>(dv), lddv, nullptr, nullptr, nullptr);
    AttnPlan P;
    const bool drop = drop_entry && p > 0.f;
    if (int rc = fwd ? plan_fwd(A, head_dim, drop, who, P) : plan_bwd(A, head_dim, drop, scratch, scratch_bytes, who, P)) return rc;
    std::string all;
    for (int i = 0; i < P.n; ++i) {
        grid_block_lds[3 * i] = (int)P.launch[i].grid; grid_block_lds[3 * i + 1] = (int)P.launch[i].block; grid_block_lds[3 * i + 2] = P.launch[i].lds;
        all += (i ? "\n" : "") + std::string(P.launch[i].name);
    }
    *n_launches = P.n;
    args_set[0] = P.lean_hw_log2; args_set[1] = P.head_splits;
    args_set[2] = P.pbuf ? (long long)(reinterpret_cast<const unsigned char *>(P.pbuf) - static_cast<const unsigned char *>(scratch)) : -1;
    snprintf(names, (size_t)names_cap, "%s", all.c_str());
    return ECGB_OK;
}

#ifdef ECGB_PROFILE
extern "C" void ecgb_debug_attn_profile(unsigned long long *out8, int reset)
{
    if (out8) (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_attn_prof), 64 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[64] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_prof), z, sizeof z); }
}
#endif

// head_dim 64, forward and backward: 2 = the lean LDS-DMA kernels (default), 1 = the round-2 LDS-DMA kernels, 0 = the register-staged kernels (tests, A/B);
// | 0x100 / 0x200 / 0x400 with mode 2: the forward / dQ / dK-dV kernel alone stays on mode 1
extern "C" int ecgb_set_attn_lean_waves(int waves)
{
    if (waves != 4 && waves != 8) { ecgb::set_error("ecgb_set_attn_lean_waves: 4 or 8"); return ECGB_ERR_INVALID; }
    g_lean_waves = waves;
    return ECGB_OK;
}
extern "C" int ecgb_set_attn_d256_pass_p(int on) { g_attn_d256_pass_p = on ? 1 : 0; return ECGB_OK; }

extern "C" int ecgb_set_attn_fwd_staging(int mode)
{
    if ((mode & 3) == 3 || (mode & ~0x703)) { ecgb::set_error("ecgb_set_attn_fwd_staging: mode 0, 1 or 2 (| 0x100 | 0x200 | 0x400)"); return ECGB_ERR_INVALID; }
    g_attn_dma = mode;
    return ECGB_OK;
}
