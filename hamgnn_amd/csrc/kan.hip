// kan.hip -- the hidden part of the B-spline KAN radial weight generators (HamGNN_pre.use_kan; reference: toolbox/efficient_kan/kan.py:78-166).
// A KANLinear is LINEAR in the expanded row phi(x) = [silu(x_i) | B_0(x_i) .. B_{nb-1}(x_i)]_i (B: cubic Cox-de Boor on feature i's own knots, order 0 the
// half-open indicator, zero outside the outermost knots; nb = G + 3 bases on G + 7 knots), so a generator  rbf -> KANLinear_0 -> .. -> h_last -> KANLinear_last  is
//     Phi = phi(h_last)   (this file: [nmlp][E][(1 + nb) h_pad], plane p of channel c at column p h_pad + c, h_pad = h_last rounded up to 16, padding = 0)
//     out = Phi W3'       (the edge kernels' radial scale: W3' takes the place of w3 / sqrt(H), plan/message_pack.py:kan_last_layer)
// No 1/sqrt(fan_in), no normalize2mom constant, no activation between layers; a value on either side of a knot is evaluated by the same formula (the splines
// are C2: which side an fp32 value lands on changes the result continuously).
//
// Per generator the caller packs (ops.KanGenerator), floats:   for every hidden layer l:  knot table [d_l][KS] | W'_l ;   then the knot table [d_last][KS] of phi(h_last).
//   knot table row (one input feature, KS = 4 (G + 7) - 6):  t_0 .. t_{G+6} | r1_j = 1 / (t_{j+1} - t_j) | r2_j = 1 / (t_{j+2} - t_j) | r3_j = 1 / (t_{j+3} - t_j)
//   W'_l  plain  : [(1 + nb) d_l][d_{l+1}] row-major, row p d_l + i = plane p of input i   (p = 0: base_weight, p >= 1: spline_weight[.., p - 1] * spline_scaler)
//         packed : MFMA A fragments [T][p][rt][lane][4]: lane (i = lane & 15, g = lane >> 4), register q <- W'[p][in = 16 T + 4 g + q][out = 16 rt + i]
#include "hg_device.h"

// phi of one value: out[0] = silu(x), out[1 + j] = B_j(x).  kt: the feature's knot table row (LDS or global).
template <int G>
__device__ __forceinline__ void kan_phi(float x, const float* __restrict__ kt, float* __restrict__ out) {
    constexpr int NK = G + 7;
    const float* t = kt;
    const float* r1 = kt + NK;
    const float* r2 = r1 + (NK - 1);
    const float* r3 = r2 + (NK - 2);
    float tk[NK], d[NK], b[NK - 1];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        tk[j] = t[j];
        d[j] = x - tk[j];
    }
#pragma unroll
    for (int j = 0; j < NK - 1; ++j) b[j] = (x >= tk[j] && x < tk[j + 1]) ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < NK - 2; ++j) b[j] = d[j] * r1[j] * b[j] - d[j + 2] * r1[j + 1] * b[j + 1];
#pragma unroll
    for (int j = 0; j < NK - 3; ++j) b[j] = d[j] * r2[j] * b[j] - d[j + 3] * r2[j + 1] * b[j + 1];
#pragma unroll
    for (int j = 0; j < NK - 4; ++j) out[1 + j] = d[j] * r3[j] * b[j] - d[j + 4] * r3[j + 1] * b[j + 1];
    out[0] = x / (1.f + __expf(-x));
}

// ------------------------------------------------------------------------------------------------ plain path (any shape)
// 16 edges per workgroup.  Per layer: phi of the 16 x d_l activations into LDS, then every thread owns (edge, 4 outputs) of the [16] x [d_{l+1}] product
// against W' read through L2 (16 lanes share an address).  Fixed summation order.
#define KAN_TE 16
template <int G>
__global__ __launch_bounds__(256) void kan_plain_kernel(const float* __restrict__ rbf, int64_t E, const float* __restrict__ blob_all, int64_t gen_stride,
                                                        int d0, int d1, int d2, int d3, int nl, int hpad, float* __restrict__ out_all, int maxd) {
    constexpr int NP = G + 4, KS = 4 * (G + 7) - 6;
    extern __shared__ float sm[];
    const int lda = maxd + 1, ldp = NP * maxd + 1;             // odd strides: conflict-free across the 16 edges
    float* act = sm;
    float* phi = sm + KAN_TE * lda;
    const float* __restrict__ w = blob_all + (int64_t)blockIdx.y * gen_stride;
    float* __restrict__ out = out_all + (int64_t)blockIdx.y * E * NP * hpad;
    const int64_t e0 = (int64_t)blockIdx.x * KAN_TE;
    const int dims[4] = {d0, d1, d2, d3};
    for (int idx = threadIdx.x; idx < KAN_TE * d0; idx += blockDim.x) {
        const int e = idx / d0, k = idx - e * d0;
        const int64_t er = e0 + e < E ? e0 + e : E - 1;        // a missing edge reads the last one (never stored)
        act[e * lda + k] = rbf[er * d0 + k];
    }
    float vals[NP];
    for (int l = 0; l < nl; ++l) {
        const int di = dims[l], dn = dims[l + 1];
        __syncthreads();
        for (int idx = threadIdx.x; idx < KAN_TE * di; idx += blockDim.x) {
            const int e = idx & (KAN_TE - 1), k = idx >> 4;
            kan_phi<G>(act[e * lda + k], w + k * KS, vals);
#pragma unroll
            for (int p = 0; p < NP; ++p) phi[e * ldp + p * di + k] = vals[p];
        }
        __syncthreads();
        const float* __restrict__ Wl = w + di * KS;
        const int F = NP * di;
        const int e = threadIdx.x & (KAN_TE - 1), o0 = 4 * (threadIdx.x >> 4);
        if (o0 < dn) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int f = 0; f < F; ++f) {
                const float xv = phi[e * ldp + f];
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (o0 + b < dn) acc[b] = fmaf(xv, Wl[f * dn + o0 + b], acc[b]);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (o0 + b < dn) act[e * lda + o0 + b] = acc[b];   // (the expansion above was the last reader of this layer's input)
        }
        w += di * KS + F * dn;
    }
    __syncthreads();
    const int dl = dims[nl], ldo = NP * hpad;                  // (ldo <= NP * maxd: maxd is a multiple of 16)
    for (int idx = threadIdx.x; idx < KAN_TE * hpad; idx += blockDim.x) {
        const int e = idx & (KAN_TE - 1), k = idx >> 4;
        if (k < dl) {
            kan_phi<G>(act[e * lda + k], w + k * KS, vals);
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p) vals[p] = 0.f;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) phi[e * ldp + p * hpad + k] = vals[p];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < KAN_TE * ldo; idx += blockDim.x) {
        const int e = idx / ldo, c = idx - e * ldo;
        if (e0 + e < E) out[(e0 + e) * ldo + c] = phi[e * ldp + c];
    }
}

// ------------------------------------------------------------------------------------------------ MFMA path: 64 -> 64 -> 64, G = 3
// Edges are the MFMA columns (16 per tile, KAN_NT tiles per wave and fragment load), as in radial_hidden_mfma_kernel: the C fragments of a layer --
// lane (i, g), register r = channel 16 rt + 4 g + r of edge i -- are expanded to phi in registers (knot tables of the generator in LDS) and feed the next
// layer as B operands in the same permuted-K order the A fragments were packed in.  Two layers hold 2 x 448 x 64 floats = 229 KB of W': neither registers
// nor LDS, so the fragments stream from L2 (1 KB per wave and 4 KAN_NT MFMAs), 448 v_mfma_f32_16x16x4_f32 per layer and tile.
#define KAN_NT 2
#define KAN_G 3
#define KAN_NP 7
#define KAN_KS 34
#define KAN_W (KAN_NP * 64 * 64)
#define KAN_KT (64 * KAN_KS)
#define KAN_STRIDE (3 * KAN_KT + 2 * KAN_W)

__device__ __forceinline__ void kan_mfma_layer(const f32x4 (&x)[KAN_NT][4], const float* __restrict__ kn, const f32x4* __restrict__ frag, int lane, int g,
                                               f32x4 (&acc)[KAN_NT][4]) {
#pragma unroll
    for (int n = 0; n < KAN_NT; ++n)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[n][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < 4; ++T) {
        // (the fragments do not depend on the tile: left alone, the compiler hoists all 224 loads of both layers out of the persistent loop and spills them)
        const f32x4* fT = frag + T * (KAN_NP * 4 * 64) + lane;
        asm volatile("" : "+v"(fT));
        float ph[KAN_NT][4][KAN_NP];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                          // (one knot row at a time: its 34 floats serve the KAN_NT tiles)
#pragma unroll
            for (int n = 0; n < KAN_NT; ++n) kan_phi<KAN_G>(x[n][T][q], kn + (16 * T + 4 * g + q) * KAN_KS, ph[n][q]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int p = 0; p < KAN_NP; ++p)
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const f32x4 a = fT[(p * 4 + rt) * 64];
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int n = 0; n < KAN_NT; ++n) acc[n][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], ph[n][q][p], acc[n][rt], 0, 0, 0);
            }
    }
}

__global__ __launch_bounds__(256) void kan_mfma_kernel(const float* __restrict__ rbf, int64_t E, const float* __restrict__ blob_all, float* __restrict__ out_all) {
    __shared__ float kn[3 * KAN_KT];                           // knot tables: layer 0 inputs | layer 1 inputs | h_last   (26 KB)
    const float* __restrict__ blob = blob_all + (int64_t)blockIdx.y * KAN_STRIDE;
    float* __restrict__ out = out_all + (int64_t)blockIdx.y * E * (KAN_NP * 64);
    for (int idx = threadIdx.x; idx < KAN_KT; idx += blockDim.x) {
        kn[idx] = blob[idx];
        kn[KAN_KT + idx] = blob[KAN_KT + KAN_W + idx];
        kn[2 * KAN_KT + idx] = blob[2 * KAN_KT + 2 * KAN_W + idx];
    }
    __syncthreads();
    const f32x4* __restrict__ f0 = reinterpret_cast<const f32x4*>(blob + KAN_KT);
    const f32x4* __restrict__ f1 = reinterpret_cast<const f32x4*>(blob + 2 * KAN_KT + KAN_W);
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int64_t ngrp = (E + 16 * KAN_NT - 1) / (16 * KAN_NT);
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < ngrp; t += (int64_t)gridDim.x * 4) {
        int64_t e[KAN_NT];
        f32x4 x[KAN_NT][4], h1[KAN_NT][4], h2[KAN_NT][4];
#pragma unroll
        for (int n = 0; n < KAN_NT; ++n) {
            e[n] = (t * KAN_NT + n) * 16 + i;
            const int64_t er = e[n] < E ? e[n] : E - 1;        // a missing edge reads the last one (never stored)
#pragma unroll
            for (int T = 0; T < 4; ++T) x[n][T] = *reinterpret_cast<const f32x4*>(rbf + er * 64 + 16 * T + 4 * g);
        }
        kan_mfma_layer(x, kn, f0, lane, g, h1);
        kan_mfma_layer(h1, kn + KAN_KT, f1, lane, g, h2);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            float ph[KAN_NT][4][KAN_NP];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int n = 0; n < KAN_NT; ++n) kan_phi<KAN_G>(h2[n][rt][r], kn + 2 * KAN_KT + (16 * rt + 4 * g + r) * KAN_KS, ph[n][r]);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int n = 0; n < KAN_NT; ++n)
                if (e[n] < E) {
#pragma unroll
                    for (int p = 0; p < KAN_NP; ++p)
                        *reinterpret_cast<f32x4*>(out + e[n] * (KAN_NP * 64) + p * 64 + 16 * rt + 4 * g) = (f32x4){ph[n][0][p], ph[n][1][p], ph[n][2][p], ph[n][3][p]};
                }
        }
    }
}

template <int G>
static int kan_launch_plain(const float* rbf, int64_t E, const float* blob, int64_t gen_stride, int nmlp, const int* d, int nl, int hpad, int maxd, float* out,
                            hipStream_t stream) {
    const size_t lds = (size_t)KAN_TE * ((size_t)(maxd + 1) + (size_t)((G + 4) * maxd + 1)) * sizeof(float);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_kan_hidden: layer too wide for the LDS-resident kernel");
    kan_plain_kernel<G><<<dim3((unsigned)((E + KAN_TE - 1) / KAN_TE), (unsigned)nmlp), 256, lds, stream>>>(rbf, E, blob, gen_stride, d[0], d[1], d[2], d[3], nl, hpad,
                                                                                                         out, maxd);
    return hg_check_launch("hg_kan_hidden");
}

extern "C" int hg_kan_hidden(const float* rbf, int64_t E, const float* blob, int64_t gen_stride, int nmlp, const int32_t* dims, int nlayers, int grid_size,
                             int packed, float* phi_out, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (nlayers < 1 || nlayers > 3) return hg_fail(-2, "hg_kan_hidden: 1..3 hidden layers supported");
    if (grid_size < 1 || grid_size > 8) return hg_fail(-2, "hg_kan_hidden: grid size 1..8 supported");
    if (nmlp < 0 || nmlp > 1024) return hg_fail(-2, "hg_kan_hidden: at most 1024 generators per launch");
    int d[4] = {0, 0, 0, 0}, maxd = 0;
    for (int l = 0; l <= nlayers; ++l) {
        d[l] = dims[l];
        if (d[l] < 1 || d[l] > 64) return hg_fail(-2, "hg_kan_hidden: layer widths 1..64 supported");
        if (d[l] > maxd) maxd = d[l];
    }
    maxd = (maxd + 15) & ~15;
    const int hpad = (d[nlayers] + 15) & ~15, NP = grid_size + 4, KS = 4 * (grid_size + 7) - 6;
    int64_t need = (int64_t)d[nlayers] * KS;
    for (int l = 0; l < nlayers; ++l) need += (int64_t)d[l] * KS + (int64_t)NP * d[l] * d[l + 1];
    if (gen_stride != need) return hg_fail(-2, "hg_kan_hidden: gen_stride does not match the packed size of these layer widths");
    const int mfma = nlayers == 2 && grid_size == KAN_G && d[0] == 64 && d[1] == 64 && d[2] == 64;
    if ((packed != 0) != (mfma != 0)) return hg_fail(-2, "hg_kan_hidden: `packed` must be 1 for 64 -> 64 -> 64 with grid size 3 (fragment order) and 0 otherwise");
    if (E <= 0 || nmlp == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (mfma) {
        const int64_t nwg = (E + 64 * KAN_NT - 1) / (64 * KAN_NT);
        kan_mfma_kernel<<<dim3((unsigned)(nwg < 2048 ? nwg : 2048), (unsigned)nmlp), 256, 0, s>>>(rbf, E, blob, phi_out);
        return hg_check_launch("hg_kan_hidden");
    }
    switch (grid_size) {
        case 1: return kan_launch_plain<1>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 2: return kan_launch_plain<2>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 3: return kan_launch_plain<3>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 4: return kan_launch_plain<4>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 5: return kan_launch_plain<5>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 6: return kan_launch_plain<6>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        case 7: return kan_launch_plain<7>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
        default: return kan_launch_plain<8>(rbf, E, blob, gen_stride, nmlp, d, nlayers, hpad, maxd, phi_out, s);
    }
}
