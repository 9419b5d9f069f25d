// spectra.hip -- density of states on a k-grid (hamgnn_amd/dos.py): the two steps after the eigen-solver (gfx950).
//   hg_mulliken_weights: per-state Mulliken weights of orbital groups, w[s, g] = wk[s] * sum_{mu in g} Re(conj(c_mu) (S c)_mu)
//   hg_dos_broaden:      D[j, g] = sum_s A(E_j, eps_s) W[s, g], A a normalised Gaussian: a GEMM whose left operand is generated in registers
// No atomics, no claim-order reduction: both kernels are bit-reproducible from launch to launch.  Callers allocate everything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hg_common.h"
#include "hamgnn_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ Mulliken weights
// One workgroup owns one state row s; wave w owns the groups g = w, w + 4, ...  The lanes of a wave stride over the orbitals of a group in the
// order of perm (lane l: entries gptr[g] + l, + 64, ...: one fma chain per lane), then a butterfly adds the 64 partial sums: a fixed tree.
// Column 0 = wk[s], column 1 + g = wk[s] * sum, columns 1 + G .. Gp - 1 = 0: every element of W is written.
__global__ __launch_bounds__(256) void mulliken_kernel(const float2* __restrict__ Cm, const float2* __restrict__ SC, int M, const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ gptr, int G, int Gp, const float* __restrict__ wk, float* __restrict__ W) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float w = wk[s];
    const float2* __restrict__ c = Cm + s * M;
    const float2* __restrict__ sc = SC + s * M;
    float* __restrict__ out = W + s * Gp;
    if (threadIdx.x == 0) out[0] = w;
    for (int col = 1 + G + (int)threadIdx.x; col < Gp; col += 256) out[col] = 0.f;
    for (int g = wave; g < G; g += 4) {                        // (wave-uniform bounds: every lane reaches every shuffle)
        const int q1 = gptr[g + 1];
        float acc = 0.f;
        for (int q = gptr[g] + lane; q < q1; q += 64) {
            const int mu = perm[q];
            const float2 a = c[mu], b = sc[mu];
            acc = fmaf(a.y, b.y, fmaf(a.x, b.x, acc));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) out[1 + g] = w * acc;
    }
}

extern "C" int hg_mulliken_weights(const float* C, const float* SC, int64_t ns, int M, const int32_t* perm, const int32_t* gptr, int G, int Gp,
                                   const float* wk, float* W, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ns <= 0) return 0;
    if (M <= 0 || G < 0 || Gp < 1 + G || ns > 2147483647LL) return hg_fail(-2, "hg_mulliken_weights: bad sizes");
    if (!C || !SC || !wk || !W || !gptr || (G > 0 && !perm)) return hg_fail(-2, "hg_mulliken_weights: null pointer");
    mulliken_kernel<<<dim3((unsigned)ns), 256, 0, (hipStream_t)stream>>>((const float2*)C, (const float2*)SC, M, perm, gptr, G, Gp, wk, W);
    return hg_check_launch("hg_mulliken_weights");
}

// ------------------------------------------------------------------------------------------------ Gaussian broadening
// One workgroup owns one (tile of 16 energies, slab of DB_NT * 16 group columns).  The states that matter to the tile are a contiguous window of
// the ascending eps: [first eps >= E_first - 6 sigma, last eps <= E_last + 6 sigma], found by two binary searches.  The window is cut into steps
// of 4 states (one v_mfma_f32_16x16x4_f32 each) and the steps are dealt to the 4 waves in contiguous quarters.  Per step a lane generates ONE
// element of the A fragment, A[energy lane & 15][state lane >> 4] = norm * exp(-((E - eps) / sigma)^2 / 2) -- the difference and the exponent in
// double, rounded to fp32 once, so the Gaussian's argument carries half an ulp -- and loads one element of W per 16-column accumulator; the A
// fragment is reused across the DB_NT accumulators.  Accumulator t holds the slab's columns DB_NT * i + t (i = lane & 15 its MFMA column), so a
// lane's DB_NT elements of W are adjacent: one 16-byte load per lane and step, a whole 256-byte row segment per 16 lanes, and one 16-byte store per
// lane and output row (Gp a multiple of 4, as dos.py pads it; any other Gp takes element loads).  The waves' partial tiles are added through LDS
// in the order ((w0 + w1) + w2) + w3.
// Tails by predication: a state slot past the window contributes a Gaussian of 0, a column >= Gp is never stored, and neither is read (their loads are
// clamped onto the window's last state / the row's last columns); rows >= ne are computed and dropped.
#define DB_NT 4                                              // 16-column accumulators per wave: 4 independent MFMA chains cover the 40-cycle latency
#define DB_WAVES 4                                           // = the 4 result registers of a lane: wave w reduces and stores register w
#define DB_BLK 16                                            // steps per block: 64 states, one eigenvalue per lane
static_assert(DB_NT == 4, "a lane's columns are one float4");
template <bool VEC>                                          // VEC: Gp a multiple of 4, rows of W and D are 16-byte aligned: a lane's columns are one float4
__global__ __launch_bounds__(64 * DB_WAVES) void dos_broaden_kernel(const float* __restrict__ eps, const float* __restrict__ W, int ns, int Gp, double E0,
                                                                    double dE, int ne, double inv_sigma, float norm, double cut, int accumulate,
                                                                    float* __restrict__ D) {
    __shared__ float part[DB_WAVES][DB_NT][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 16, c0 = blockIdx.y * (16 * DB_NT);
    const int jl = j0 + 15 < ne ? j0 + 15 : ne - 1;
    const double lo = E0 + (double)j0 * dE - cut, hi = E0 + (double)jl * dE + cut;
    int a = 0, b = ns;
    while (a < b) {                                            // first state with eps >= lo
        const int m = (a + b) >> 1;
        if ((double)eps[m] < lo) a = m + 1; else b = m;
    }
    const int s_lo = a;
    b = ns;
    while (a < b) {                                            // first state with eps > hi
        const int m = (a + b) >> 1;
        if ((double)eps[m] <= hi) a = m + 1; else b = m;
    }
    const int s_hi = a;
    const int nsteps = (s_hi - s_lo + 3) >> 2;
    if (nsteps == 0 && accumulate) return;                     // (block-uniform) an empty window leaves D alone
    const int chunk = (nsteps + DB_WAVES - 1) / DB_WAVES;
    const int st0 = wave * chunk, st1 = st0 + chunk < nsteps ? st0 + chunk : nsteps;
    const double Ej = E0 + (double)(j0 + (lane & 15)) * dE;
    const int kq = lane >> 4, col = c0 + DB_NT * (lane & 15);   // first of this lane's DB_NT adjacent columns
    f32x4 acc[DB_NT];
#pragma unroll
    for (int t = 0; t < DB_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one step = this lane's state s = s_lo + 4 st + kq: its eigenvalue and its DB_NT elements of W.  No branch around a load: a state slot past the
    // window reads the window's last state and a column past Gp the row's last ones (always inside W), the slot's Gaussian is set to 0 and columns
    // >= Gp are never stored.  Steps go in blocks of DB_BLK: the block's 4 DB_BLK eigenvalues are ONE coalesced load (lane l: state 4 sb + l) handed
    // round by a lane shuffle, and the block's W loads are all requested before its first Gaussian is formed.
    const int colc = VEC ? (col < Gp ? col : Gp - DB_NT) : 0;
    auto load_w = [&](int st, float (&bv)[DB_NT]) {
        int s = s_lo + 4 * st + kq;
        s = s < s_hi ? s : s_hi - 1;
        const float* __restrict__ w = W + (int64_t)s * Gp;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w + colc, 16));
            bv[0] = v.x, bv[1] = v.y, bv[2] = v.z, bv[3] = v.w;
        } else {
#pragma unroll
            for (int t = 0; t < DB_NT; ++t) bv[t] = w[col + t < Gp ? col + t : Gp - 1];
        }
    };
    auto load_eps = [&](int sb) {
        const int s = s_lo + 4 * sb + lane;
        return eps[s < s_hi ? s : s_hi - 1];
    };
    auto step = [&](int st, float e, const float (&bv)[DB_NT]) {
        const double x = (Ej - (double)e) * inv_sigma;
        float av = norm * expf((float)(-0.5 * x * x));
        av = s_lo + 4 * st + kq < s_hi ? av : 0.f;
#pragma unroll
        for (int t = 0; t < DB_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
    };
    int sb = st0;                                              // (all bounds below are wave-uniform; st0 < st1 implies a window that is not empty)
    for (; sb + DB_BLK <= st1; sb += DB_BLK) {
        const float e64 = load_eps(sb);
        float bv[DB_BLK][DB_NT];
#pragma unroll
        for (int i = 0; i < DB_BLK; ++i) load_w(sb + i, bv[i]);
#pragma unroll
        for (int i = 0; i < DB_BLK; ++i) step(sb + i, __shfl(e64, 4 * i + kq, 64), bv[i]);
    }
    if (sb < st1) {
        const float e64 = load_eps(sb);
        for (int i = 0; sb + i < st1; ++i) {
            float bv[DB_NT];
            load_w(sb + i, bv);
            step(sb + i, __shfl(e64, 4 * i + kq, 64), bv);
        }
    }
#pragma unroll
    for (int t = 0; t < DB_NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][t][r][lane] = acc[t][r];
    __syncthreads();
    {                                                          // C/D map of a 16x16 tile: MFMA column = lane & 15, row = 4 (lane >> 4) + r; wave w adds and stores rows r = w
        const int r = wave, row = j0 + 4 * kq + r;
        float v[DB_NT];
#pragma unroll
        for (int t = 0; t < DB_NT; ++t) {
            v[t] = part[0][t][r][lane];
#pragma unroll
            for (int w2 = 1; w2 < DB_WAVES; ++w2) v[t] += part[w2][t][r][lane];
        }
        if (row < ne) {
            float* dst = D + (int64_t)row * Gp + col;
            if (VEC) {
                if (col < Gp) {
                    float4 o = make_float4(v[0], v[1], v[2], v[3]);
                    if (accumulate) {
                        const float4 old = *reinterpret_cast<const float4*>(dst);
                        o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
                    }
                    *reinterpret_cast<float4*>(dst) = o;
                }
            } else {
#pragma unroll
                for (int t = 0; t < DB_NT; ++t)
                    if (col + t < Gp) dst[t] = accumulate ? dst[t] + v[t] : v[t];
            }
        }
    }
}

extern "C" int hg_dos_broaden(const float* eps, const float* W, int64_t ns, int Gp, double E0, double dE, int ne, double sigma, int accumulate,
                              float* D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ne <= 0 || Gp <= 0) return 0;
    if (!(sigma > 0.0) || !(dE > 0.0) || ns < 0 || ns > 2147483647LL - 8 || !D || (ns > 0 && (!eps || !W)) || (((uintptr_t)W | (uintptr_t)D) & 15))
        return hg_fail(-2, "hg_dos_broaden: bad arguments (sigma and dE must be positive, ns < 2^31, W and D 16-byte aligned)");
    const unsigned gx = (unsigned)((ne + 15) / 16), gy = (unsigned)((Gp + 16 * DB_NT - 1) / (16 * DB_NT));
    if (gy > 65535u) return hg_fail(-2, "hg_dos_broaden: too many group columns");
    const float norm = (float)(1.0 / (sigma * 2.5066282746310002));      // 1 / (sigma sqrt(2 pi))
    if ((Gp & 3) == 0)
        dos_broaden_kernel<true><<<dim3(gx, gy), 64 * DB_WAVES, 0, (hipStream_t)stream>>>(eps, W, (int)ns, Gp, E0, dE, ne, 1.0 / sigma, norm, 6.0 * sigma,
                                                                                           accumulate ? 1 : 0, D);
    else
        dos_broaden_kernel<false><<<dim3(gx, gy), 64 * DB_WAVES, 0, (hipStream_t)stream>>>(eps, W, (int)ns, Gp, E0, dE, ne, 1.0 / sigma, norm, 6.0 * sigma,
                                                                                            accumulate ? 1 : 0, D);
    return hg_check_launch("hg_dos_broaden");
}
