// row_ops.hip -- the memory-bound kernels on feature rows around the fused edge kernel (gfx950): segmented node scatter, gate and norm-activation with
// their adjoints, row adds, planar layout conversion, embedding lookup; the MFMA probe of bench.py; and the host-only runtime of the library (error
// string, launch check, version, scratch query).  See include/hamgnn_hip.h for the reference op cluster each entry point replaces.
#include <stdio.h>
#include <string.h>
#include "hg_device.h"

static thread_local char g_err[512] = "";

int hg_fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "unknown");
    return code;
}
int hg_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return -1;
    }
    return 0;
}
int hg_lds_attr_once(unsigned char* done, int dev, const void* kernel, int bytes) {
    if (dev < 0 || dev >= HG_MAX_DEVICES) return hg_fail(-3, "device index out of range");
    if (__atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) return 0;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return hg_fail(-3, hipGetErrorString(e));
    __atomic_store_n(&done[dev], (unsigned char)1, __ATOMIC_RELEASE);
    return 0;
}
extern "C" const char* hg_last_error(void) { return g_err; }
extern "C" int hg_version(void) { return 2; }

// Workspace query ("no hidden allocation on the hot path -- workspace size is queried").  No entry point of this library
// allocates: outputs and scratch are caller-provided.  Those that need scratch beyond their documented outputs report its size here;
// every other entry point returns 0.  Host-only: callable without a GPU.
extern "C" int64_t hg_scratch_bytes(const char* entry_point, int64_t rows, int arg) {
    if (!entry_point || rows < 0) return -1;
    auto is = [&](const char* n) { const char* a = entry_point; while (*a && *a == *n) { ++a; ++n; } return *a == 0 && *n == 0; };
    if (is("hg_edge_geometry")) return rows * 4 * (int64_t)sizeof(float);              // ang_scratch [E][4]
    if (is("hg_zero_point_shift")) return 2 * (int64_t)(arg > 0 ? arg : 256) * (int64_t)sizeof(double);   // partial_scratch [2 nparts]
    if (is("hg_linear_wgrad")) return ((rows + 1023) / 1024) * (int64_t)(arg > 0 ? arg : 0) * 1024 * (int64_t)sizeof(float);   // partial [chunks][arg = nunits][16][64]
    if (is("hg_kgrad_elements")) return hg_kgrad_chunks(arg) > 1 ? hg_kgrad_chunks(arg) * rows * 6 * (int64_t)sizeof(float) : 0;   // part [chunks(arg = n_edges)][rows = n_pairs][6]
    return 0;
}

// ------------------------------------------------------------------------------------------------ segmented node scatter
// Wavefront segmented reduce over the receiver CSR: one block per node; a lane owns one 16-byte column of the row, so a wavefront reads
// 1 KiB of each incoming message row with one coalesced float4 load; the edge list is walked four edges at a time (four independent
// index loads, then four row loads in flight) and summed in list order -- fixed order, hence bit-reproducible, unlike the atomics of
// torch_scatter.scatter (hamgnn/nn/convolution.py:147-149).
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ msg, int64_t ms, const int64_t* __restrict__ rowptr,
                                                          const int64_t* __restrict__ perm, int Dp, float* __restrict__ out, int64_t os) {
    const int64_t n = blockIdx.x;
    const int64_t q0 = rowptr[n], q1 = rowptr[n + 1];
    for (int p = 4 * threadIdx.x; p < Dp; p += 4 * blockDim.x) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        int64_t q = q0;
        for (; q + 4 <= q1; q += 4) {
            const int64_t e0 = perm[q], e1 = perm[q + 1], e2 = perm[q + 2], e3 = perm[q + 3];
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(msg + e0 * ms + p), v1 = *reinterpret_cast<const f32x4*>(msg + e1 * ms + p);
            const f32x4 v2 = *reinterpret_cast<const f32x4*>(msg + e2 * ms + p), v3 = *reinterpret_cast<const f32x4*>(msg + e3 * ms + p);
            acc = (((acc + v0) + v1) + v2) + v3;
        }
        for (; q < q1; ++q) acc += *reinterpret_cast<const f32x4*>(msg + perm[q] * ms + p);
        *reinterpret_cast<f32x4*>(out + n * os + p) = acc;
    }
}

extern "C" int hg_segment_sum(const float* msg, int64_t msg_stride, const int64_t* rowptr, const int64_t* perm, int64_t N, int Dp,
                              float* out, int64_t out_stride, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (N <= 0) return 0;
    if ((Dp & 3) || (msg_stride & 3) || (out_stride & 3) || ((reinterpret_cast<uintptr_t>(msg) | reinterpret_cast<uintptr_t>(out)) & 15))
        return hg_fail(-2, "hg_segment_sum: rows must be multiples of 4 floats and 16-byte aligned (planar rows are)");
    segment_sum_kernel<<<dim3((unsigned)N), 256, 0, (hipStream_t)stream>>>(msg, msg_stride, rowptr, perm, Dp, out, out_stride);
    return hg_check_launch("hg_segment_sum");
}

// ------------------------------------------------------------------------------------------------ gate / adds / layout
// (not rowprog.hip's rp_act: log1pf / tanhf and threshold 20 here, hardware exp / log / divide and threshold 15 there -- merging the two changes results)
__device__ __forceinline__ float hg_act(float x, int id, const float* __restrict__ cst) {
    switch (id) {
        case 1: return cst[1] * ((x > 20.f ? x : log1pf(__expf(x))) - 0.6931471805599453f);     // shifted softplus
        case 2: return cst[2] * tanhf(x);
        case 3: return cst[3] * x / (1.f + __expf(-x));
        case 4: return cst[4] * fabsf(x);
        default: return x;
    }
}

// One wave per row, no block barriers.  Phase A: the row's DISTINCT activated scalars (the 0e / 0o scalars and the gate channels: 263 of
// the 1012 inputs for set-A) go through their activation once, into a wave-private LDS strip; phase B: every output element is a plain
// input or an activated scalar, times its gate's activated value -- look-ups only.  (The r1 kernel evaluated softplus = log1pf(expf)
// once per OUTPUT element, i.e. (2l+1) times per gate channel: the E-row gates of the head ran compute-bound at 1.8 TB/s.)
// act_tab: int32[nact][2] = {input index, act id};  out_tab: int32[Dout][2] = {source code, gate code}: source code = input index, or
// 0x40000000 | act slot; gate code = act slot or -1; source code -1 = structural zero.
#define HG_GATE_WAVES 4
__global__ __launch_bounds__(256) void gate_kernel(const float* __restrict__ x, int64_t xs, const int2* __restrict__ act_tab, int nact,
                                                   const int2* __restrict__ out_tab, int Dout, const float* __restrict__ cst, int64_t rows,
                                                   float* __restrict__ out, int64_t os) {
    extern __shared__ __attribute__((aligned(16))) int sm_i[];
    int2* __restrict__ s_out = reinterpret_cast<int2*>(sm_i);                           // [Dout]
    int2* __restrict__ s_act = s_out + Dout;                                            // [nact]
    float* __restrict__ s_val = reinterpret_cast<float*>(s_act + nact);                 // [HG_GATE_WAVES][nact]
    for (int i = threadIdx.x; i < Dout; i += blockDim.x) s_out[i] = out_tab[i];
    for (int i = threadIdx.x; i < nact; i += blockDim.x) s_act[i] = act_tab[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* __restrict__ av = s_val + wave * nact;
    float c[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) c[i] = cst[i];
    for (int64_t r = (int64_t)blockIdx.x * HG_GATE_WAVES + wave; r < rows; r += (int64_t)gridDim.x * HG_GATE_WAVES) {
        const float* __restrict__ xr = x + r * xs;
        for (int i = lane; i < nact; i += 64) {
            const int2 t = s_act[i];
            av[i] = hg_act(xr[t.x], t.y, c);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float* __restrict__ orow = out + r * os;
#pragma unroll 4
        for (int p = lane; p < Dout; p += 64) {
            const int2 t = s_out[p];
            float v = 0.f;
            if (t.x >= 0) {
                v = (t.x & 0x40000000) ? av[t.x & 0x3fffffff] : xr[t.x];
                if (t.y >= 0) v *= av[t.y];
            }
            orow[p] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                       // the strip is rewritten by the next row
    }
}

extern "C" int hg_gate(const float* x, int64_t x_stride, const int32_t* act_tab, int nact, const int32_t* out_tab, int Dout, const float* consts,
                       int64_t rows, float* out, int64_t out_stride, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    if (nact < 0 || Dout <= 0) return hg_fail(-2, "hg_gate: bad table sizes");
    const size_t lds = sizeof(int) * (2 * (size_t)Dout + 2 * (size_t)nact + (size_t)HG_GATE_WAVES * (size_t)nact);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_gate: row too wide for the LDS tables");
    const int64_t want = (rows + HG_GATE_WAVES - 1) / HG_GATE_WAVES;
    const int64_t blocks = want < 256 * 8 ? want : 256 * 8;    // persistent: the tables are staged once per block
    gate_kernel<<<dim3((unsigned)blocks), 256, lds, (hipStream_t)stream>>>(x, x_stride, (const int2*)act_tab, nact, (const int2*)out_tab, Dout,
                                                                           consts, rows, out, out_stride);
    return hg_check_launch("hg_gate");
}

// Backward of the gate (data gradient): with out[p] = f(x[src]) (activated scalar), x[src] * act(x[gate]) (gated component),
//   gx[src]  = gy[p] * f'(x[src])                       activated scalar
//   gx[src]  = gy[p] * act(x[gate])                     gated component
//   gx[gate] = act'(x[gate]) * sum_p gy[p] * x[src(p)]  over the components the gate channel multiplies
// Same tables and the same wave-per-row structure as gate_kernel: activations and their derivatives once per row into wave-private LDS
// strips, the per-gate sums accumulate there (ds_add_f32 inside one wave: no barrier), input columns no output reads get 0.
__device__ __forceinline__ float hg_act_grad(float x, int id, const float* __restrict__ cst) {
    switch (id) {
        case 1: return cst[1] / (1.f + __expf(-x));                                             // d/dx softplus = sigmoid
        case 2: { const float t = tanhf(x); return cst[2] * (1.f - t * t); }
        case 3: { const float s = 1.f / (1.f + __expf(-x)); return cst[3] * s * (1.f + x * (1.f - s)); }
        case 4: return cst[4] * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
        default: return 1.f;
    }
}
__global__ __launch_bounds__(256) void gate_backward_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ gy, int64_t gs,
                                                            const int2* __restrict__ act_tab, int nact, const int2* __restrict__ out_tab, int Dout,
                                                            const float* __restrict__ cst, int64_t rows, int Din, float* __restrict__ gx, int64_t gxs) {
    extern __shared__ __attribute__((aligned(16))) int sm_i[];
    int2* __restrict__ s_out = reinterpret_cast<int2*>(sm_i);                           // [Dout]
    int2* __restrict__ s_act = s_out + Dout;                                            // [nact]
    float* __restrict__ s_val = reinterpret_cast<float*>(s_act + nact);                 // [HG_GATE_WAVES][3 nact + Din]: act, act', gate sums, the gx row
    for (int i = threadIdx.x; i < Dout; i += blockDim.x) s_out[i] = out_tab[i];
    for (int i = threadIdx.x; i < nact; i += blockDim.x) s_act[i] = act_tab[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* __restrict__ av = s_val + wave * (3 * nact + Din);
    float* __restrict__ dv = av + nact;
    float* __restrict__ sv = dv + nact;
    float* __restrict__ row = sv + nact;                       // the gradient row is assembled in LDS (every column written once, then
    float c[5];                                                // gate columns accumulate), and leaves as one coalesced copy
#pragma unroll
    for (int i = 0; i < 5; ++i) c[i] = cst[i];
    for (int64_t r = (int64_t)blockIdx.x * HG_GATE_WAVES + wave; r < rows; r += (int64_t)gridDim.x * HG_GATE_WAVES) {
        const float* __restrict__ xr = x + r * xs;
        const float* __restrict__ gr = gy + r * gs;
        for (int i = lane; i < Din; i += 64) row[i] = 0.f;
        for (int i = lane; i < nact; i += 64) {
            const int2 t = s_act[i];
            av[i] = hg_act(xr[t.x], t.y, c);
            dv[i] = hg_act_grad(xr[t.x], t.y, c);
            sv[i] = 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int p = lane; p < Dout; p += 64) {
            const int2 t = s_out[p];
            if (t.x < 0) continue;
            const float g = gr[p];
            if (t.x & 0x40000000) {                            // activated scalar: slot -> its input column
                const int slot = t.x & 0x3fffffff;
                float v = g * dv[slot];
                if (t.y >= 0) {                                // (an activated scalar that is gated as well: not produced by the planner)
                    atomicAdd(&sv[t.y], g * av[slot]);
                    v *= av[t.y];
                }
                row[s_act[slot].x] = v;
            } else if (t.y >= 0) {                             // gated component
                row[t.x] = g * av[t.y];
                atomicAdd(&sv[t.y], g * xr[t.x]);
            } else {
                row[t.x] = g;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < nact; i += 64) row[s_act[i].x] += sv[i] * dv[i];          // gate channels: act'(x) * sum (plain scalars: + 0)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float* __restrict__ orow = gx + r * gxs;
        for (int i = lane; i < Din; i += 64) orow[i] = row[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                       // the strips are rewritten by the next row
    }
}

extern "C" int hg_gate_backward(const float* x, int64_t x_stride, const float* gy, int64_t gy_stride, const int32_t* act_tab, int nact,
                                const int32_t* out_tab, int Dout, const float* consts, int64_t rows, int Din, float* gx, int64_t gx_stride,
                                void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    if (nact < 0 || Dout <= 0 || Din <= 0) return hg_fail(-2, "hg_gate_backward: bad table sizes");
    const size_t lds = sizeof(int) * (2 * (size_t)Dout + 2 * (size_t)nact + (size_t)HG_GATE_WAVES * (3 * (size_t)nact + (size_t)Din));
    if (lds > 64 * 1024) return hg_fail(-2, "hg_gate_backward: row too wide for the LDS tables");
    const int64_t want = (rows + HG_GATE_WAVES - 1) / HG_GATE_WAVES;
    const int64_t blocks = want < 256 * 8 ? want : 256 * 8;
    gate_backward_kernel<<<dim3((unsigned)blocks), 256, lds, (hipStream_t)stream>>>(x, x_stride, gy, gy_stride, (const int2*)act_tab, nact,
                                                                                    (const int2*)out_tab, Dout, consts, rows, Din, gx, gx_stride);
    return hg_check_launch("hg_gate_backward");
}

// e3nn NormActivation of a ResidualBlock with nonlinearity_type = "norm" (hamgnn/nn/interaction_blocks.py:311-330: scalar nonlinearity ssp AS GIVEN,
// normalize = True, epsilon = 1e-8, no bias) on planar rows: every irrep copy (channel u of block b: components x[off + a * mulp + u], a < 2 l + 1) is
// scaled by ssp(n) / n with n = sqrt(max(sum_a x_a^2, eps^2)).  chan_tab int32[nchan][2] = {offset of the channel's first component, component
// stride (mulp) | ncomp << 16}; the channel-padding slots of a planar row (no table entry) are written as zeros.  One thread per (row, channel).
__device__ __forceinline__ float hg_ssp(float x) { return (x > 20.f ? x : log1pf(__expf(x))) - 0.69314718055994531f; }
// The two factors of the kernels below, ssp(n) / n and (sigmoid(n) - ssp(n) / n) / n.  log1pf(__expf(n)) and ln 2 are both 0.69 for small n and the difference
// cancels (1.4e-5 of the scale at n = 1e-2, a scale of 0 instead of 0.5 at the clamp n = 1e-8), so below HG_SSP_SERIES the factors come from their series
// ln(1 + e^n) = ln 2 + n/2 + n^2/8 - n^4/192 + ...: 1/2 + n/8 - n^3/192 (next term n^5/2880: 7e-9 of the value at the threshold) and 1/8 - n^2/64 (next term
// n^4/576: 1e-6 of the factor, which scales a term that is n/4 of the gradient: 4e-8); above the threshold the direct form loses 1e-7 / (n/2), below 2e-6.
#define HG_SSP_SERIES 0.1f
__device__ __forceinline__ float hg_ssp_over_n(float n) {
    return n < HG_SSP_SERIES ? fmaf(n, fmaf(n * n, -1.f / 192.f, 0.125f), 0.5f) : hg_ssp(n) / n;
}
__device__ __forceinline__ float hg_dssp_over_n(float n, float sc) {       // (sigmoid(n) - sc) / n with sc = hg_ssp_over_n(n)
    return n < HG_SSP_SERIES ? fmaf(n * n, -1.f / 64.f, 0.125f) : (1.f / (1.f + __expf(-n)) - sc) / n;
}
__global__ void norm_act_kernel(const float* __restrict__ x, int64_t xs, const int2* __restrict__ chan_tab, int nchan, float eps2, int64_t rows,
                                float* __restrict__ out, int64_t os) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nchan) return;
    const int64_t r = i / nchan;
    const int2 t = chan_tab[(int)(i - r * nchan)];
    const int st = t.y & 0xffff, nc = t.y >> 16;
    const float* __restrict__ xr = x + r * xs + t.x;
    float n2 = 0.f;
    for (int a = 0; a < nc; ++a) n2 = fmaf(xr[a * st], xr[a * st], n2);
    n2 = n2 < eps2 ? eps2 : n2;
    const float n = sqrtf(n2), sc = hg_ssp_over_n(n);
    float* __restrict__ o = out + r * os + t.x;
    for (int a = 0; a < nc; ++a) o[a * st] = sc * xr[a * st];
}

extern "C" int hg_norm_act(const float* x, int64_t x_stride, const int32_t* chan_tab, int nchan, float eps, int64_t rows, float* out,
                           int64_t out_stride, int D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    if (nchan <= 0 || D <= 0) return hg_fail(-2, "hg_norm_act: bad table sizes");
    if (hipMemsetAsync(out, 0, sizeof(float) * (size_t)rows * (size_t)out_stride, (hipStream_t)stream) != hipSuccess)      // channel-padding slots
        return hg_fail(-3, "hg_norm_act: memset failed");
    const int64_t n = rows * nchan;
    norm_act_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(x, x_stride, (const int2*)chan_tab, nchan, eps * eps, rows, out, out_stride);
    return hg_check_launch("hg_norm_act");
}

// its data gradient: y_a = s(n) / n * x_a  =>  gx_a = s / n * gy_a + x_a (sum_b gy_b x_b) (s'(n) - s / n) / n^2   (n > eps; below the clamp n is a
// constant and only the first term is left); s = ssp, s' = sigmoid
__global__ void norm_act_backward_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ gy, int64_t gs, const int2* __restrict__ chan_tab,
                                         int nchan, float eps2, int64_t rows, float* __restrict__ gx, int64_t gxs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nchan) return;
    const int64_t r = i / nchan;
    const int2 t = chan_tab[(int)(i - r * nchan)];
    const int st = t.y & 0xffff, nc = t.y >> 16;
    const float* __restrict__ xr = x + r * xs + t.x;
    const float* __restrict__ gr = gy + r * gs + t.x;
    float n2 = 0.f, dot = 0.f;
    for (int a = 0; a < nc; ++a) {
        n2 = fmaf(xr[a * st], xr[a * st], n2);
        dot = fmaf(gr[a * st], xr[a * st], dot);
    }
    const bool clamped = n2 < eps2;
    n2 = clamped ? eps2 : n2;
    const float n = sqrtf(n2), sc = hg_ssp_over_n(n);
    const float k = clamped ? 0.f : dot * hg_dssp_over_n(n, sc) / n;
    float* __restrict__ o = gx + r * gxs + t.x;
    for (int a = 0; a < nc; ++a) o[a * st] = fmaf(k, xr[a * st], sc * gr[a * st]);
}

extern "C" int hg_norm_act_backward(const float* x, int64_t x_stride, const float* gy, int64_t gy_stride, const int32_t* chan_tab, int nchan, float eps,
                                    int64_t rows, float* gx, int64_t gx_stride, int D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    if (nchan <= 0 || D <= 0) return hg_fail(-2, "hg_norm_act_backward: bad table sizes");
    if (hipMemsetAsync(gx, 0, sizeof(float) * (size_t)rows * (size_t)gx_stride, (hipStream_t)stream) != hipSuccess)
        return hg_fail(-3, "hg_norm_act_backward: memset failed");
    const int64_t n = rows * nchan;
    norm_act_backward_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(x, x_stride, gy, gy_stride, (const int2*)chan_tab, nchan,
                                                                                               eps * eps, rows, gx, gx_stride);
    return hg_check_launch("hg_norm_act_backward");
}

__global__ void add_rows_kernel(const float* __restrict__ a, int64_t sa, const float* __restrict__ b, int64_t sb,
                                const float* __restrict__ c, int64_t sc, int64_t rows, int D, float* __restrict__ out, int64_t so) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const int64_t r = i / D;
    const int p = (int)(i - r * D);
    float v = a[r * sa + p] + b[r * sb + p];
    if (c) v += c[r * sc + p];
    out[r * so + p] = v;
}

extern "C" int hg_add_rows(const float* a, int64_t sa, const float* b, int64_t sb, const float* c, int64_t sc, int64_t rows, int D,
                           float* out, int64_t so, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    add_rows_kernel<<<dim3((unsigned)((rows * D + 255) / 256)), 256, 0, (hipStream_t)stream>>>(a, sa, b, sb, c, sc, rows, D, out, so);
    return hg_check_launch("hg_add_rows");
}

__global__ void to_planar_kernel(const float* __restrict__ x, int64_t rows, int D, const int* __restrict__ map, float* __restrict__ out, int Dp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const int64_t r = i / D;
    const int k = (int)(i - r * D);
    out[r * Dp + map[k]] = x[i];
}
__global__ void from_planar_kernel(const float* __restrict__ xp, int64_t rows, int Dp, const int* __restrict__ map, float* __restrict__ out, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const int64_t r = i / D;
    const int k = (int)(i - r * D);
    out[i] = map[k] >= 0 ? xp[r * Dp + map[k]] : 0.f;            // -1: structural zero (column gathers of the gradient layouts)
}
extern "C" int hg_to_planar(const float* x, int64_t rows, int D, const int32_t* map, float* out, int Dp, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    (void)hipMemsetAsync(out, 0, sizeof(float) * (size_t)rows * Dp, (hipStream_t)stream);
    to_planar_kernel<<<dim3((unsigned)((rows * D + 255) / 256)), 256, 0, (hipStream_t)stream>>>(x, rows, D, map, out, Dp);
    return hg_check_launch("hg_to_planar");
}
extern "C" int hg_from_planar(const float* xp, int64_t rows, int Dp, const int32_t* map, float* out, int D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    from_planar_kernel<<<dim3((unsigned)((rows * D + 255) / 256)), 256, 0, (hipStream_t)stream>>>(xp, rows, Dp, map, out, D);
    return hg_check_launch("hg_from_planar");
}

__global__ void embed_lookup_kernel(const float* __restrict__ Ta, const float* __restrict__ Tb, const int64_t* __restrict__ z,
                                    const int64_t* __restrict__ ia, const int64_t* __restrict__ ib, int64_t rows, int T, int Tp,
                                    float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Tp) return;
    const int64_t r = i / Tp;
    const int t = (int)(i - r * Tp);
    float v = 0.f;
    if (t < T) {
        v = Ta[z[ia ? ia[r] : r] * T + t];
        if (Tb) v += Tb[z[ib ? ib[r] : r] * T + t];
    }
    out[i] = v;
}
extern "C" int hg_embed_lookup(const float* Ta, const float* Tb, const int64_t* z, const int64_t* idx_a, const int64_t* idx_b,
                               int64_t rows, int T, int Tp, float* out, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (rows <= 0) return 0;
    embed_lookup_kernel<<<dim3((unsigned)((rows * Tp + 255) / 256)), 256, 0, (hipStream_t)stream>>>(Ta, Tb, z, idx_a, idx_b, rows, T, Tp, out);
    return hg_check_launch("hg_embed_lookup");
}

// ------------------------------------------------------------------------------------------------ measurement aid (bench.py roofline)
// What the fp32 matrix pipe sustains on THIS device at THIS moment: every wave issues `iters` x 8 v_mfma_f32_16x16x4_f32 on eight independent
// accumulators, operands from the caller's (random) buffer, two waves per SIMD on every CU -- nothing else in the loop.  The chip clocks to its
// power budget on non-trivial data (MI355X_MICROARCH.md, DVFS), so the nominal 157.3 TFLOP/s is quoted beside this number, not replaced by it.
__global__ __launch_bounds__(256, 2) void mfma_probe_kernel(const float* __restrict__ in, float* __restrict__ out, int iters) {
    const int tid = blockIdx.x * 256 + threadIdx.x;
    float a[8], b[8];
    f32x4 acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a[k] = in[(tid * 16 + k) & 0xffff];
        b[k] = in[(tid * 16 + 8 + k) & 0xffff];
        acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[(k + 3) & 7], acc[k], 0, 0, 0);
    }
    f32x4 s = acc[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += acc[k];
    out[tid] = s[0] + s[1] + s[2] + s[3];
}

extern "C" int hg_mfma_probe(const float* in65536, float* out, int nblocks, int iters, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (nblocks <= 0 || iters <= 0) return hg_fail(-2, "hg_mfma_probe: nblocks and iters must be positive");
    mfma_probe_kernel<<<dim3((unsigned)nblocks), 256, 0, (hipStream_t)stream>>>(in65536, out, iters);
    return hg_check_launch("hg_mfma_probe");
}
