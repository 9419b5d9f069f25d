// radial.hip -- the hidden layers of the radial weight generators (RadialBasisEdgeEncoding -> the MLPs of the tensor-product weights; gfx950) and the
// device-side refill of the split-half-precision twins of their last layer (csrc/tp_is.hip).  kan.hip holds the KAN generators.
// See include/hamgnn_hip.h for the reference op cluster each entry point replaces.
#include "hg_device.h"

// ------------------------------------------------------------------------------------------------ radial hidden layers
// 64 edges per workgroup; activations and the current layer's weights in LDS; each thread owns a 4 (edges) x 4 (outputs)
// register tile per pass.  act(x) = cst * silu(x) (e3nn normalize2mom(silu)); weights already carry 1/sqrt(h_in).
#define RH_TE 64
__global__ __launch_bounds__(256) void radial_hidden_kernel(const float* __restrict__ rbf, int64_t E, const float* __restrict__ W,
                                                            int d0, int d1, int d2, int d3, int nlayers, float cst,
                                                            float* __restrict__ out, int maxd) {
    extern __shared__ float sm[];
    const int ld = maxd + 1;                                   // +1: conflict-free column access
    float* buf0 = sm;
    float* buf1 = sm + RH_TE * ld;
    float* wsm = sm + 2 * RH_TE * ld;                          // [di][dn]
    const int64_t e0 = (int64_t)blockIdx.x * RH_TE;
    const int dims[4] = {d0, d1, d2, d3};
    for (int i = threadIdx.x; i < RH_TE * d0; i += blockDim.x) {
        const int e = i / d0, k = i - e * d0;
        buf0[e * ld + k] = (e0 + e < E) ? rbf[(e0 + e) * d0 + k] : 0.f;
    }
    const float* w = W;
    float* in = buf0;
    float* ot = buf1;
    for (int l = 0; l < nlayers; ++l) {
        const int di = dims[l], dn = dims[l + 1];
        __syncthreads();
        for (int i = threadIdx.x; i < di * dn; i += blockDim.x) wsm[i] = w[i];
        __syncthreads();
        const int ng = (dn + 3) >> 2;                          // output groups of 4
        for (int tile = threadIdx.x; tile < (RH_TE / 4) * ng; tile += blockDim.x) {
            const int eg = tile / ng, og = tile - eg * ng;
            float acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
            for (int k = 0; k < di; ++k) {
                float xv[4], wv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) xv[a] = in[(4 * eg + a) * ld + k];
#pragma unroll
                for (int b = 0; b < 4; ++b) wv[b] = (4 * og + b < dn) ? wsm[k * dn + 4 * og + b] : 0.f;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xv[a], wv[b], acc[a][b]);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (4 * og + b < dn) {
                        const float v = acc[a][b];
                        ot[(4 * eg + a) * ld + 4 * og + b] = cst * v / (1.f + __expf(-v));
                    }
        }
        w += di * dn;
        float* t = in; in = ot; ot = t;
    }
    __syncthreads();
    const int dl = dims[nlayers];
    for (int i = threadIdx.x; i < RH_TE * dl; i += blockDim.x) {
        const int e = i / dl, j = i - e * dl;
        if (e0 + e < E) out[(e0 + e) * dl + j] = in[e * ld + j];
    }
}

// MFMA version for the shipped shape (64 radial functions -> 64 -> 64): edges are the MFMA columns (16 per wave tile), both weight
// matrices live in registers as A fragments (2 x 16 float4 per lane) for the whole persistent loop, and layer 1's C fragments
// feed layer 2 as B operands directly (permuted-K packing, as in tp_fused.hip): 128 v_mfma_f32_16x16x4_f32 per 16 edges, one
// coalesced read of the rbf row, one write of the hidden row.  (The LDS/VALU kernel above ran at 21 TFLOP/s, 0.64 ms per launch.)
__device__ __forceinline__ f32x4 rh_silu(f32x4 v, float cst) {
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = cst * v[r] / (1.f + __expf(-v[r]));
    return o;
}
__global__ __launch_bounds__(256) void radial_hidden_mfma_kernel(const float* __restrict__ rbf, int64_t E, const float* __restrict__ W_all, float cst,
                                                                 float* __restrict__ out_all) {
    // blockIdx.y: which MLP of a batch of 64 -> 64 -> 64 weight generators that share the radial basis rows (hg_radial_hidden_multi: all
    // 13 generators of a 3-layer backbone in ONE launch -- the basis rows come from HBM once, the other readers hit L2 / Infinity Cache)
    const float* __restrict__ W = W_all + (int64_t)blockIdx.y * 8192;
    float* __restrict__ out = out_all + (int64_t)blockIdx.y * E * 64;
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    // A fragments: lane (i, g), tile (rt, T), register q  <-  W[in = 16 T + 4 g + q][out = 16 rt + i]   (W row-major [in][out])
    f32x4 a1[4][4], a2[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a1[rt][T][q] = W[(16 * T + 4 * g + q) * 64 + 16 * rt + i];
                a2[rt][T][q] = W[4096 + (16 * T + 4 * g + q) * 64 + 16 * rt + i];
            }
    const int64_t ntile = (E + 15) >> 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < ntile; t += (int64_t)gridDim.x * 4) {
        const int64_t e = t * 16 + i;
        const int64_t er = e < E ? e : E - 1;
        f32x4 x[4];
#pragma unroll
        for (int T = 0; T < 4; ++T) x[T] = *reinterpret_cast<const f32x4*>(rbf + er * 64 + 16 * T + 4 * g);
        f32x4 h1[4], h2[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int T = 0; T < 4; ++T)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[rt][T][q], x[T][q], acc, 0, 0, 0);
            h1[rt] = rh_silu(acc, cst);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int T = 0; T < 4; ++T)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[rt][T][q], h1[T][q], acc, 0, 0, 0);
            h2[rt] = rh_silu(acc, cst);
        }
        if (e < E) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) *reinterpret_cast<f32x4*>(out + e * 64 + 16 * rt + 4 * g) = h2[rt];
        }
    }
}

extern "C" int hg_radial_hidden(const float* rbf, int64_t E, const float* weights, const int32_t* dims, int nlayers, float act_cst,
                                float* h_out, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0) return 0;
    if (nlayers < 1 || nlayers > 3) return hg_fail(-2, "hg_radial_hidden: 1..3 hidden layers supported");
    if (nlayers == 2 && dims[0] == 64 && dims[1] == 64 && dims[2] == 64) {
        const int64_t nwg = (E + 63) / 64;
        const unsigned grid = (unsigned)(nwg < 2048 ? nwg : 2048);            // persistent: the weight fragments are loaded once per wave
        radial_hidden_mfma_kernel<<<dim3(grid), 256, 0, (hipStream_t)stream>>>(rbf, E, weights, act_cst, h_out);
        return hg_check_launch("hg_radial_hidden");
    }
    int d[4] = {0, 0, 0, 0}, maxd = 0, maxw = 0;
    for (int i = 0; i <= nlayers; ++i) { d[i] = dims[i]; if (d[i] > maxd) maxd = d[i]; }
    for (int i = 0; i < nlayers; ++i) if (d[i] * d[i + 1] > maxw) maxw = d[i] * d[i + 1];
    const size_t lds = (2 * RH_TE * (size_t)(maxd + 1) + (size_t)maxw) * sizeof(float);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_radial_hidden: layer too wide for the LDS-resident kernel");
    radial_hidden_kernel<<<dim3((unsigned)((E + RH_TE - 1) / RH_TE)), 256, lds, (hipStream_t)stream>>>(rbf, E, weights, d[0], d[1], d[2], d[3], nlayers, act_cst, h_out, maxd);
    return hg_check_launch("hg_radial_hidden");
}

extern "C" int hg_radial_hidden_multi(const float* rbf, int64_t E, const float* weights, int nmlp, float act_cst, float* h_out, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0 || nmlp <= 0) return 0;
    if (nmlp > 1024) return hg_fail(-2, "hg_radial_hidden_multi: at most 1024 generators per launch");
    const int64_t nwg = (E + 63) / 64;
    const unsigned grid = (unsigned)(nwg < 2048 ? nwg : 2048);
    radial_hidden_mfma_kernel<<<dim3(grid, (unsigned)nmlp), 256, 0, (hipStream_t)stream>>>(rbf, E, weights, act_cst, h_out);
    return hg_check_launch("hg_radial_hidden_multi");
}

// ---- split-half-precision twins of the radial weights (csrc/tp_is.hip: radial scale on v_mfma_f32_16x16x32_f16; plan/program.py:w3_split_fill) refilled ON THE DEVICE after a
// device-side repack (training): pair k = the two fp32 weights w[se[k]], w[so[k]] that share a dword of the twin; hi = f16(x 2^s), lo = f16((x 2^s - hi) 2^11), written as packed
// pairs at dh[k] / dl[k]; max |x 2^s| into maxabs (non-negative floats order like their bit patterns) for the host's range check.  One launch per program (the torch-op version: 18).
__global__ __launch_bounds__(256) void w3_split_refill_kernel(float* __restrict__ w, const int64_t* __restrict__ se, const int64_t* __restrict__ so, const int64_t* __restrict__ dh,
                                                              const int64_t* __restrict__ dl, int64_t n, float scale, float lo_scale, float* __restrict__ maxabs) {
    float m = 0.f;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const float xe = w[se[k]] * scale, xo = w[so[k]] * scale;
        const _Float16 he = (_Float16)xe, ho = (_Float16)xo;
        const _Float16 le = (_Float16)((xe - (float)he) * lo_scale), lo = (_Float16)((xo - (float)ho) * lo_scale);
        unsigned short a, b;
        __builtin_memcpy(&a, &he, 2); __builtin_memcpy(&b, &ho, 2);
        reinterpret_cast<unsigned*>(w)[dh[k]] = (unsigned)a | ((unsigned)b << 16);
        __builtin_memcpy(&a, &le, 2); __builtin_memcpy(&b, &lo, 2);
        reinterpret_cast<unsigned*>(w)[dl[k]] = (unsigned)a | ((unsigned)b << 16);
        m = fmaxf(m, fmaxf(fabsf(xe), fabsf(xo)));
    }
    if (!(m == m)) m = __int_as_float(0x7f800000);              // NaN weights: beyond any range
    atomicMax(reinterpret_cast<unsigned*>(maxabs), __float_as_uint(m));
}

extern "C" int hg_w3_split_refill(float* weights, const int64_t* src_even, const int64_t* src_odd, const int64_t* dst_hi, const int64_t* dst_lo, int64_t npairs,
                                  float scale, float lo_scale, float* maxabs, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (npairs <= 0) return 0;
    if (!weights || !src_even || !src_odd || !dst_hi || !dst_lo || !maxabs) return hg_fail(-2, "hg_w3_split_refill: null pointer");
    if (hipMemsetAsync(maxabs, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return hg_fail(-3, "hg_w3_split_refill: memset failed");
    const int64_t blocks = (npairs + 255) / 256;
    w3_split_refill_kernel<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), 256, 0, (hipStream_t)stream>>>(weights, src_even, src_odd, dst_hi, dst_lo, npairs, scale, lo_scale, maxabs);
    return hg_check_launch("hg_w3_split_refill");
}
