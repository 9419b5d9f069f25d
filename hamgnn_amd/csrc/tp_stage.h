// tp_stage.h -- operand staging (gather + frame rotation / LDS-DMA), epilogue (un-rotation + planar store) and the launch-argument block
// of the input-stationary edge kernel csrc/tp_is.hip (dynamic work claiming, register-chained row-tile chunks).
// Hand-written HIP for gfx950 (CDNA4).
#pragma once
#include "hg_device.h"
#include "tp_epilogue_map.h"

// the 16 edges' hidden rows of a phase's radial MLP as B operands of v_mfma_f32_16x16x32_f16: x = hi + lo (csrc/tp_is.hip, plan/program.py:w3_split_fill)
// c0 = 2^-(sw + sh): undoes the weights' exponent and the tile's
struct IsHidden { f16x8 hi[2], lo[2]; float c0; };
// The hidden rows are scaled by 2^sh before the split, sh chosen PER 16-EDGE TILE AND PHASE from the rows themselves (= plan.split_h_exp): the tile's largest
// |h| lands in [2^IS_SPLIT_H_TOP, 2^(IS_SPLIT_H_TOP + 1)).  Every finite row is handled: 2^-88 <= max |h| < 2^113 exactly as described, below that range the
// clamped exponent only lets the flush set in earlier, above it the halves overflow to what the fp32 form gives there as well (inf / NaN).
#define IS_SPLIT_H_TOP 12
#define IS_SPLIT_H_MIN (-100)
#define IS_SPLIT_H_MAX 100

#ifndef IS_NW
#define IS_NW 4                  // waves of a workgroup (all on the same 16 edges); plan.py:IS_WAVES.  6 = three waves per SIMD (experiment)
#endif
#define IS_NT (64 * IS_NW)
#ifndef IS_NW_LITE
#define IS_NW_LITE 8             // lite_mode programs (tp_is_kernel<SPLIT, LITE = true>): 8 waves per workgroup = four waves per SIMD at 128 VGPRs;
#endif                           // plan.py:IS_WAVES_LITE

struct IsArgs {
    const float* src[4];
    int64_t sstride[4];
    const float* h2[2];
    int hidden;
    const float* wig;
    int nW;
    int wig_off[8];
    float* out;
    int64_t ostride;
    int64_t rows;
    int nseg;                    // single-part launches: the whole program (split launches read these per part, see IS_PART_I32)
    int nphase;
    int trash_off;               // float offsets inside the workgroup's LDS
    int stage_off;
    int ctr_off;                 // work-claim counter (one dword)
    int rowtab_off;              // row table of GEMM2's output rows (ints): LDS float offset of every row's centre column, see plan.IsSchedule
    int rowtab_begin;            // first entry / entries of this part in the global table
    int rowtab_len;
    int tile_shift;              // split launches: this wave's private tile copy (floats added to every tile offset)
    int s_split;                 // the program carries the split-half-precision twins of its W3 blocks (part record [12]): radial scales on the f16 matrix pipe
    float s_scale;               // 2^-sw: undoes the scaling of the twins (part record [13]); the hidden rows' exponent is the tile's (IsHidden.c0)
    const int64_t* idx[4];       // per source slot: row gather (NULL: row = edge)
    int rot_mask;                // bit i: source i holds GLOBAL-frame rows that are rotated into the edge frame while staged
    const int64_t* eperm;        // tile slot -> edge (NULL: identity).  Receiver-major order for launches whose output is scattered onto the receivers
    const int32_t* run_id;       // fused scatter (NULL: one output row per edge): slot -> index of its run of equal receivers inside the tile = the
                                 // output row that takes the run's sum (convolution.py:147-149 as a segmented reduce in the epilogue); -1: no output
};

// Fused node scatter: the 16 slots of a tile lie along a DPP row (lane = 16 g + slot).  seg_masks: for the Hillis-Steele steps d = 1, 2, 4, 8 of a
// segmented inclusive scan, 1.0 where slot el adds the partial sum of slot el - d (no run head in (el - d, el]), else 0.0; `last`: the slot closes
// its run (its lane holds the run's sum after the scan).  Fixed order of additions: bit-reproducible, unlike the reference's atomics.
struct IsScan {
    float m[4];
    bool last;
    int row;
};
template <int CTRL>
__device__ __forceinline__ int is_dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float is_dpp_f(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)); }
__device__ __forceinline__ IsScan is_scan_setup(int rid, int el) {
    IsScan sc;
    sc.row = rid;
    const int prev = is_dpp_i<0x111>(rid), next = is_dpp_i<0x101>(rid);          // row_shr:1 / row_shl:1 (0 beyond the row's ends)
    int f = (el == 0 || prev != rid) ? 1 : 0;                                     // run head
    sc.last = el == 15 || next != rid;
    sc.m[0] = f ? 0.f : 1.f;
    int f1 = f | (el < 1 ? 1 : is_dpp_i<0x111>(f));
    sc.m[1] = f1 ? 0.f : 1.f;
    int f2 = f1 | (el < 2 ? 1 : is_dpp_i<0x112>(f1));
    sc.m[2] = f2 ? 0.f : 1.f;
    int f4 = f2 | (el < 4 ? 1 : is_dpp_i<0x114>(f2));
    sc.m[3] = f4 ? 0.f : 1.f;
    return sc;
}
__device__ __forceinline__ float is_seg_scan(float x, const IsScan& sc) {
    x = fmaf(sc.m[0], is_dpp_f<0x111>(x), x);
    x = fmaf(sc.m[1], is_dpp_f<0x112>(x), x);
    x = fmaf(sc.m[2], is_dpp_f<0x114>(x), x);
    x = fmaf(sc.m[3], is_dpp_f<0x118>(x), x);
    return x;
}

// the four channels of a lane go out as one 16-byte store -- or, AT (split launches) and the segment flagged SEG_ATOMIC, as four hardware float adds
template <bool AT>
__device__ __forceinline__ void is_store4(float* __restrict__ p, f32x4 v, int flags) {
    if constexpr (AT) {
        if (flags & SEG_ATOMIC) {
#pragma unroll
            for (int k = 0; k < 4; ++k) unsafeAtomicAdd(p + k, v[k]);
            return;
        }
    }
    *reinterpret_cast<f32x4*>(p) = v;
}

// un-rotate (optional) + planar store of one segment, rows split over the four waves; D blocks staged in `dst` (see kernel)
template <int LK, int NW, bool AT = false>
__device__ __forceinline__ void epilogue_is(const IsArgs& A, const float* __restrict__ tile, const float* __restrict__ dstage, int mul_k,
                                            int out_off, int out_mulp, int flags, int64_t e, bool valid_in, int wave, int lane, const IsScan& sc) {
    bool valid = valid_in;
    constexpr int NCO = 2 * LK + 1;
    const int g = lane >> 4, el = lane & 15;
    const int rowstride = NCO * 16 + 4;
    const float* __restrict__ tl = tile + el;
    // fused scatter: the output row is the run's row, written by the slot that closes the run after the segmented scan over the 16 slots
    const bool red = A.run_id != nullptr;
    if (red) valid = sc.last && sc.row >= 0;
    float* __restrict__ ob = A.out + (red ? (int64_t)(sc.row >= 0 ? sc.row : 0) : e) * A.ostride + out_off;
    const int wend = mul_k + ((flags >> 8) & 0xff);            // + channel-padding slots of the planar block (last chunk only)
    // work unit = one float4 of the segment's planar block, unit j = a * nq + quad (tp_epilogue_map.h): a wave step serves four consecutive units,
    // one per lane group, and a wave a contiguous range of steps -- 64 contiguous bytes per edge and wave instruction where the components
    // follow each other without a gap, so the memory side sees whole sectors (interleaving the channels of one component over the waves
    // tripled the HBM write traffic: WRITE_SIZE 1.39 GB vs 0.46 GB of output per 131 072 edges).  Units of 16 channels per component
    // left the lane groups beyond a narrow segment's channels idle: 106 wave steps per tile of the set-A blocks where these take 65.
    const IsEpiMap em = is_epi_map(NCO, wend, NW, wave);
    // a lane owns FOUR consecutive channels of one (edge, component): 4 NCO tile reads in flight, one 16-byte store -- a wave writes 16 edges x
    // 64 contiguous bytes per request (r3: a dword per lane, four requests for the same bytes)
    if (LK > 0 && (flags & SEG_UNROTATE) && (flags & SEG_CENTRE)) {
        // every item that fed this tile wrote its centre column (m = 0) only (plan/schedule_is.py: SEG_CENTRE; the first ConvBlock of a backbone, whose node rows
        // are 0e and whose edge rows hold the m = 0 component of Y^l): out[a] = D[LK][a] t[LK] -- one tile read and one product per channel where the full
        // un-rotation takes 2 LK + 1, and the kernel has staged row LK of the Wigner block alone: image [a][edge]
        const float* __restrict__ dl = dstage + el;
        const float* __restrict__ tc = tl + LK * 16;
#pragma unroll 1
        for (int s = em.s_begin; s < em.s_end; ++s) {
            int a, w;
            if (!is_epi_unit(em, s, g, a, w)) continue;
            const float dc = dl[a * 16];
            f32x4 acc;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = w + k < mul_k ? dc * tc[(w + k) * rowstride] : 0.f;
            if (red) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = is_seg_scan(acc[k], sc);
            }
            if (valid) is_store4<AT>(ob + a * out_mulp + w, acc, flags);
        }
    } else if (flags & SEG_UNROTATE) {
        const float* __restrict__ dl = dstage + el;
#pragma unroll 1
        for (int s = em.s_begin; s < em.s_end; ++s) {
            int a, w;
            if (!is_epi_unit(em, s, g, a, w)) continue;
            float dc[NCO];
#pragma unroll
            for (int m = 0; m < NCO; ++m) dc[m] = dl[(m * NCO + a) * 16];
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* __restrict__ tw = tl + (w + k < mul_k ? w + k : 0) * rowstride;
#pragma unroll
                for (int m = 0; m < NCO; ++m) acc[k] = fmaf(dc[m], tw[m * 16], acc[k]);
                acc[k] = w + k < mul_k ? acc[k] : 0.f;
            }
            if (red) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = is_seg_scan(acc[k], sc);
            }
            if (valid) is_store4<AT>(ob + a * out_mulp + w, acc, flags);
        }
    } else {
#pragma unroll 1
        for (int s = em.s_begin; s < em.s_end; ++s) {
            int a, w;
            if (!is_epi_unit(em, s, g, a, w)) continue;
            f32x4 acc;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = w + k < mul_k ? tl[(w + k) * rowstride + a * 16] : 0.f;
            if (red) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = is_seg_scan(acc[k], sc);
            }
            if (valid) is_store4<AT>(ob + a * out_mulp + w, acc, flags);
        }
    }
}


#ifndef HG_STAGE_FUSE_LMAX
#define HG_STAGE_FUSE_LMAX 6     // both node sources rotated in one pass up to this l 
#endif
// piece index t -> (component a, channel piece p): t / P1 through the reciprocal (t < 2^9, P1 <= 16: (t + 0.5) / P1 is never within 0.03 of an
// integer, so the float product rounds to the right side); an integer division per piece cost as much as the piece's own loads + FMAs at l = 0
#define HG_DIV_P1(t) ((int)(((float)(t) + 0.5f) * inv_P1))
#ifndef HG_STAGE_U
#define HG_STAGE_U(L) 1          // measured (profiles/r02_tp_is_experiments.md): 2-4 pieces in flight per step are SLOWER (8.39 vs 8.13 ms)
#endif
// Stage one input block (all its sources) of the workgroup's 16 edges: image offset(piece p = a * P1 + s, row e) = 64 p + 4 e per source.
//   plain source  : rows are already in the edge frame -> LDS-DMA, the four waves share the DMA instructions;
//   rotated source: rows are node features in the global frame, gathered by idx[] and multiplied by D^l(R_e) on the way in
//                   (x'[a] = sum_b D[a][b] x[b], hamgnn_amd/so3.py) -- ONCE per edge, input block and launch, which replaces the
//                   separate hg_rotate_gather pass and the materialised per-edge copies xs', xd' of the node rows.
template <int L, int NW>
__device__ __forceinline__ void stage_block(const IsArgs& A, const int* __restrict__ P, float* __restrict__ stage, int64_t erow, int wave, int lane) {
    if constexpr (NW > 4) asm volatile("" : "+v"(erow));       // 128-register budget: the rows' addresses are formed per block (hoisted out of the
                                                               // phase loop they were spilled: a scratch reload per staged piece)
    constexpr int N = 2 * L + 1;
    const int s0 = P[0], s1 = P[1], in_off = P[2], in_mulp = P[3], nsrc = P[5];
    const int g = lane >> 4, el = lane & 15;
    const int P1 = in_mulp >> 2;
    const float inv_P1 = 1.0f / (float)P1;
    const int Pfull = N * P1;
    const int nj = (Pfull + 3) >> 2;
    const bool rot0 = (A.rot_mask >> s0) & 1, rot1 = nsrc == 2 && ((A.rot_mask >> s1) & 1);
    if (rot0 && rot1 && (NW <= 4 || L <= 3) && L <= HG_STAGE_FUSE_LMAX) {
        // sender and receiver rows of the node branch share the edge's Wigner row: one output piece t = a * P1 + p (component a,
        // channels 4p..4p+3) of BOTH sources per (wave, g) slot and step -- 2 N float4 loads of the node rows + the N entries of
        // row a in flight together, 2 N float4 FMAs, two ds_write_b128 straight into the operand images
        const int64_t* __restrict__ ix0 = hg_pick4(A.idx, s0);
        const int64_t* __restrict__ ix1 = hg_pick4(A.idx, s1);
        const int64_t r0 = ix0 ? ix0[erow] : erow, r1 = ix1 ? ix1[erow] : erow;
        const float* __restrict__ row0 = hg_pick4(A.src, s0) + r0 * hg_pick4(A.sstride, s0) + in_off;
        const float* __restrict__ row1 = hg_pick4(A.src, s1) + r1 * hg_pick4(A.sstride, s1) + in_off;
        const float* __restrict__ D = A.wig + erow * A.nW + A.wig_off[L];
        float* __restrict__ d0 = stage + P[6] + el * 4;
        float* __restrict__ d1 = stage + P[7] + el * 4;
        // U output pieces per step (register budget by l): the node rows come from the Infinity Cache / HBM (35 MB of node rows do not
        // fit an XCD's L2), so every step of this loop exposes ~1 us of latency -- with 2 N float4 + N scalar loads of U pieces in flight
        // instead of one piece's
        constexpr int U = HG_STAGE_U(L);
#pragma unroll 1
        for (int t0 = 4 * wave + g; t0 < Pfull; t0 += 4 * NW * U) {
            f32x4 v0[U][N], v1[U][N];
            float d[U][N];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int t = t0 + 4 * NW * u;
                t = t < Pfull ? t : t0;                        // tail: re-read the first piece (result dropped below)
                const int a = HG_DIV_P1(t), p = t - a * P1;
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    v0[u][b] = *reinterpret_cast<const f32x4*>(row0 + b * in_mulp + 4 * p);
                    v1[u][b] = *reinterpret_cast<const f32x4*>(row1 + b * in_mulp + 4 * p);
                    d[u][b] = D[a * N + b];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 4 * NW * u;
                if (t < Pfull) {
                    f32x4 acc0 = d[u][0] * v0[u][0], acc1 = d[u][0] * v1[u][0];
#pragma unroll
                    for (int b = 1; b < N; ++b) {
                        acc0 += d[u][b] * v0[u][b];
                        acc1 += d[u][b] * v1[u][b];
                    }
                    *reinterpret_cast<f32x4*>(d0 + t * 64) = acc0;
                    *reinterpret_cast<f32x4*>(d1 + t * 64) = acc1;
                }
            }
        }
        return;
    }
    for (int si = 0; si < nsrc; ++si) {
        const int sidx = si ? s1 : s0;
        const int64_t* __restrict__ ix = hg_pick4(A.idx, sidx);
        const int64_t r = ix ? ix[erow] : erow;
        const float* __restrict__ row = hg_pick4(A.src, sidx) + r * hg_pick4(A.sstride, sidx) + in_off;
        float* __restrict__ dst = stage + (si ? P[7] : P[6]);
        if (si ? rot1 : rot0) {
            const float* __restrict__ D = A.wig + erow * A.nW + A.wig_off[L];
#pragma unroll 1
            for (int t = 4 * wave + g; t < Pfull; t += 4 * NW) {
                const int a = HG_DIV_P1(t), p = t - a * P1;
                f32x4 v[N];
                float d[N];
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    v[b] = *reinterpret_cast<const f32x4*>(row + b * in_mulp + 4 * p);
                    d[b] = D[a * N + b];
                }
                f32x4 acc = d[0] * v[0];
#pragma unroll
                for (int b = 1; b < N; ++b) acc += d[b] * v[b];
                *reinterpret_cast<f32x4*>(dst + t * 64 + el * 4) = acc;
            }
        } else {
#pragma unroll 1
            for (int j = wave; j < nj; j += NW) {              // the waves share the block's DMA instructions
                int p = 4 * j + g;
                p = p < Pfull ? p : Pfull - 1;
                hg_dma16(row + 4 * p, dst + j * 256);
            }
        }
    }
}

#define SEG_NEWBATCH (1 << 16)
