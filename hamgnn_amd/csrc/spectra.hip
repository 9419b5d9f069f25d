// spectra.hip -- density of states on a k-grid (hamgnn_amd/dos.py): the steps after the eigen-solver (gfx950).
//   hg_mulliken_weights: per-state Mulliken weights of orbital groups, w[s, g] = wk[s] * sum_{mu in g} Re(conj(c_mu) (S c)_mu)
//   hg_dos_broaden:      D[j, g] = sum_s A(E_j, eps_s) W[s, g], A a normalised Gaussian: a GEMM whose left operand is generated in registers
//   hg_dos_tetra:        the same GEMM with the linear tetrahedron method's corner weights (DOS or number of states) as the left operand
//   hg_bond_weights:     per-state bond weights (COOP / COHP), w[s, g] = wk[s] * sum_{bonds of g} Re(phase c_i^+ X_bond c_j) from the real-space rows
//   hg_density_rows:     the density matrix sampled on the rows of the crystal graph, P[e][a, b] = sum_s f_s Re(phase conj(c_ia) c_jb): an SDDMM over the states
//   hg_kgrad_elements:   matrix elements of dX(k)/dk between pairs of states, out[p, alpha] = sum_e i rvec[e, alpha] phase c_bra^+ X_e c_ket: band velocities
// No atomics, no claim-order reduction: all kernels are bit-reproducible from launch to launch.  Callers allocate everything.
#include "hg_device.h"

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

// ------------------------------------------------------------------------------------------------ the tile of the two DOS GEMMs
// D[j, g] = sum_s A[j, s] W[s, g]: dos_broaden_kernel and dos_tetra_kernel differ in the window of states and in how a lane generates its element of A;
// the rest is here.  One workgroup owns one (tile of 16 energies, slab of DB_NT * 16 group columns).  The states that matter to the tile are cut into
// steps of 4 (one v_mfma_f32_16x16x4_f32 each: lane l holds A[energy l & 15][state l >> 4]) and the steps are dealt to the 4 waves in contiguous quarters.
// Per step a lane loads one element of W per 16-column accumulator; the A fragment is reused across the DB_NT accumulators.  Accumulator t holds the
// slab's columns DB_NT * i + t (i = lane & 15 its MFMA column), so a lane's DB_NT elements of W are adjacent: one 16-byte load per lane and step, a whole
// 256-byte row segment per 16 lanes, and one 16-byte store per lane and output row (VEC: Gp a multiple of 4, as dos.py pads it, rows of W and D 16-byte
// aligned; any other Gp takes element loads and stores).  C/D map of a 16x16 tile: MFMA column = lane & 15, row = 4 (lane >> 4) + r.  The waves' partial
// tiles are added through LDS in the order ((w0 + w1) + w2) + w3; wave w adds and stores the rows r = w.
// Tails by predication: a state slot past the window contributes an A element of 0, a column >= Gp is never stored, and neither is read (their loads are
// clamped onto the window's last state / the row's last columns, always inside W); rows >= ne are computed and dropped.
#define DB_NT 4                                              // 16-column accumulators per wave: 4 independent MFMA chains cover the 40-cycle latency
#define DB_WAVES 4                                           // = the 4 result registers of a lane: wave w reduces and stores register w
static_assert(DB_NT == 4, "a lane's columns are one float4");
struct DosTile {
    int lane, wave, sl, kq;                                  // sl = lane & 15: the lane's energy of a step and its MFMA column; kq = lane >> 4: its state of a step, its row quarter
    int j0, col, colc;                                       // first energy of the tile; first of the lane's DB_NT adjacent columns; the same clamped for VEC loads
};
template <bool VEC>
__device__ __forceinline__ DosTile dos_tile(int Gp) {
    DosTile t;
    t.lane = threadIdx.x & 63, t.wave = threadIdx.x >> 6, t.sl = t.lane & 15, t.kq = t.lane >> 4;
    t.j0 = blockIdx.x * 16, t.col = blockIdx.y * (16 * DB_NT) + DB_NT * t.sl;
    t.colc = VEC ? (t.col < Gp ? t.col : Gp - DB_NT) : 0;
    return t;
}
// the steps [st0, st1) of this wave: contiguous quarters of the nsteps (wave-uniform)
__device__ __forceinline__ void dos_wave_steps(const DosTile& t, int nsteps, int& st0, int& st1) {
    const int chunk = (nsteps + DB_WAVES - 1) / DB_WAVES;
    st0 = t.wave * chunk, st1 = st0 + chunk < nsteps ? st0 + chunk : nsteps;
}
// the lane's DB_NT columns of the row w of W
template <bool VEC>
__device__ __forceinline__ void dos_load_w(const float* __restrict__ w, const DosTile& t, int Gp, float (&bv)[DB_NT]) {
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w + t.colc, 16));
        bv[0] = v.x, bv[1] = v.y, bv[2] = v.z, bv[3] = v.w;
    } else {
#pragma unroll
        for (int c = 0; c < DB_NT; ++c) bv[c] = w[t.col + c < Gp ? t.col + c : Gp - 1];
    }
}
// the waves' partial tiles to LDS, their sum in the fixed order, the store (accumulate: added to what D holds)
template <bool VEC>
__device__ __forceinline__ void dos_epilogue(const f32x4 (&acc)[DB_NT], const DosTile& t, int ne, int Gp, int accumulate, float* __restrict__ D) {
    __shared__ float part[DB_WAVES][DB_NT][4][64];
#pragma unroll
    for (int c = 0; c < DB_NT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[t.wave][c][r][t.lane] = acc[c][r];
    __syncthreads();
    const int r = t.wave, row = t.j0 + 4 * t.kq + r;
    float v[DB_NT];
#pragma unroll
    for (int c = 0; c < DB_NT; ++c) {
        v[c] = part[0][c][r][t.lane];
#pragma unroll
        for (int w2 = 1; w2 < DB_WAVES; ++w2) v[c] += part[w2][c][r][t.lane];
    }
    if (row >= ne) return;
    float* dst = D + (int64_t)row * Gp + t.col;
    if (VEC) {
        if (t.col < Gp) {
            float4 o = make_float4(v[0], v[1], v[2], v[3]);
            if (accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(dst);
                o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
            }
            *reinterpret_cast<float4*>(dst) = o;
        }
    } else {
#pragma unroll
        for (int c = 0; c < DB_NT; ++c)
            if (t.col + c < Gp) dst[c] = accumulate ? dst[c] + v[c] : v[c];
    }
}
// grid of both kernels: energy tiles on x, column slabs on y; false where the slabs exceed the grid's y limit
static bool dos_grid(int ne, int Gp, dim3& grid) {
    grid = dim3((unsigned)((ne + 15) / 16), (unsigned)((Gp + 16 * DB_NT - 1) / (16 * DB_NT)));
    return grid.y <= 65535u;
}
// launch of kernel_<VEC>: VEC where the rows of W and D can be read as float4
#define HG_DOS_LAUNCH(kernel_, Gp_, grid_, stream_, ...)                                                       \
    do {                                                                                                       \
        if (((Gp_) & 3) == 0) kernel_<true><<<grid_, 64 * DB_WAVES, 0, (hipStream_t)(stream_)>>>(__VA_ARGS__); \
        else kernel_<false><<<grid_, 64 * DB_WAVES, 0, (hipStream_t)(stream_)>>>(__VA_ARGS__);                 \
    } while (0)

// ------------------------------------------------------------------------------------------------ Gaussian broadening
// The tile, the W loads, the tails and the epilogue are the DOS tile's (above).  The states that matter to the tile are a contiguous window of the
// ascending eps: [first eps >= E_first - 6 sigma, last eps <= E_last + 6 sigma], found by two binary searches.  Per step a lane generates ONE element of
// the A fragment, A[energy lane & 15][state lane >> 4] = norm * exp(-((E - eps) / sigma)^2 / 2) -- the difference and the exponent in double, rounded to
// fp32 once, so the Gaussian's argument carries half an ulp.
#define DB_BLK 16                                            // steps per block: 64 states, one eigenvalue per lane
template <bool VEC>
__global__ __launch_bounds__(64 * DB_WAVES) void dos_broaden_kernel(const float* __restrict__ eps, const float* __restrict__ W, int ns, int Gp, double E0,
                                                                    double dE, int ne, double inv_sigma, float norm, double cut, int accumulate,
                                                                    float* __restrict__ D) {
    const DosTile tl = dos_tile<VEC>(Gp);
    const int lane = tl.lane, kq = tl.kq, j0 = tl.j0;
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
    int st0, st1;
    dos_wave_steps(tl, nsteps, st0, st1);
    const double Ej = E0 + (double)(j0 + (lane & 15)) * dE;
    f32x4 acc[DB_NT] = {};
    // one step = this lane's state s = s_lo + 4 st + kq: its eigenvalue and its DB_NT elements of W.  No branch around a load (the tile's tails).  Steps
    // go in blocks of DB_BLK: the block's 4 DB_BLK eigenvalues are ONE coalesced load (lane l: state 4 sb + l) handed round by a lane shuffle, and the
    // block's W loads are all requested before its first Gaussian is formed.
    auto load_w = [&](int st, float (&bv)[DB_NT]) {
        int s = s_lo + 4 * st + kq;
        s = s < s_hi ? s : s_hi - 1;
        dos_load_w<VEC>(W + (int64_t)s * Gp, tl, Gp, bv);
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
    dos_epilogue<VEC>(acc, tl, ne, Gp, accumulate, D);
}

extern "C" int hg_dos_broaden(const float* eps, const float* W, int64_t ns, int Gp, double E0, double dE, int ne, double sigma, int accumulate,
                              float* D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ne <= 0 || Gp <= 0) return 0;
    if (!(sigma > 0.0) || !(dE > 0.0) || ns < 0 || ns > 2147483647LL - 8 || !D || (ns > 0 && (!eps || !W)) || (((uintptr_t)W | (uintptr_t)D) & 15))
        return hg_fail(-2, "hg_dos_broaden: bad arguments (sigma and dE must be positive, ns < 2^31, W and D 16-byte aligned)");
    dim3 grid;
    if (!dos_grid(ne, Gp, grid)) return hg_fail(-2, "hg_dos_broaden: too many group columns");
    const float norm = (float)(1.0 / (sigma * 2.5066282746310002));      // 1 / (sigma sqrt(2 pi))
    HG_DOS_LAUNCH(dos_broaden_kernel, Gp, grid, stream, eps, W, (int)ns, Gp, E0, dE, ne, 1.0 / sigma, norm, 6.0 * sigma, accumulate ? 1 : 0, D);
    return hg_check_launch("hg_dos_broaden");
}

// ------------------------------------------------------------------------------------------------ linear tetrahedron method
// The weights (Bloechl, Jepsen, Andersen 1994; the same text stands in hamgnn_amd/dos.py and include/hamgnn_hip.h).  Inside a tetrahedron of weight v
// the band energy and the projection weight are linear.  Corner energies sorted e1 <= e2 <= e3 <= e4 (ties keep the corner order), e_ij = e_i - e_j,
// q = v / 4, a = E - e1, b = E - e2, c = e3 - E, d = e4 - E.  Corner weight of the DOS, c_i(E) = g_T(E) * (barycentric coordinate i of the centroid of
// the cross-section at E), and of the number of states, w_i(E) = integral of c_i up to E:
//   flat (e4 - e1 < dE): a delta at the mean m of the four: DOS q max(0, 1 - |E - m| / dE) / dE per corner (on the grid: cloud-in-cell between the
//        two energies that bracket m) if E0 <= m <= E0 + (ne - 1) dE, else 0;  number of states: q per corner where E >= m, else 0;
//   E <= e1: 0;   E >= e4: 0 (DOS), q per corner (number of states);
//   e1 < E < e2:  f_j = a / e_j1;  DOS  c_1 = (v f2 f3 / e41) (3 - f2 - f3 - f4), c_j = (v f2 f3 / e41) f_j;
//                 states  C = q f2 f3 f4:  w_1 = C (4 - f2 - f3 - f4), w_j = C f_j;
//   e2 <= E < e3: C1 = q a^2 / (e41 e31), C2 = q a b c / (e41 e32 e31), C3 = q b^2 d / (e42 e32 e41);
//                 w_1 = C1 + (C1 + C2) c / e31 + (C1 + C2 + C3) d / e41,   w_2 = C1 + C2 + C3 + (C2 + C3) c / e32 + C3 d / e42,
//                 w_3 = (C1 + C2) a / e31 + (C2 + C3) b / e32,             w_4 = (C1 + C2 + C3) a / e41 + C3 b / e42;
//                 DOS: their derivatives, term by term (C1' = 2 q a / (e41 e31), C2' = q (b c + a c - a b) / (e41 e32 e31), C3' = q (2 b d - b^2) /
//                 (e42 e32 e41)): no e21 in a denominator, so e1 = e2 forms no 0 / 0;
//   e3 <= E < e4: h_j = d / e_4j;  DOS  c_4 = (v h1 h2 / e43) (3 - h1 - h2 - h3), c_j = (v h1 h2 / e43) h_j;
//                 states  C = q h1 h2 h3:  w_4 = q - C (4 - h1 - h2 - h3), w_j = q - C h_j.
// A branch is entered only where its interval is not empty, so every denominator it uses is positive.  All of it in double from the fp32 eigenvalues.
__device__ __forceinline__ double tetra_corner(double e1, double e2, double e3, double e4, int r, double E, double v, int mode, double dE, double g_lo,
                                               double g_hi) {
    const double q = 0.25 * v;
    if (e4 - e1 < dE) {
        const double m = 0.25 * (((e1 + e2) + e3) + e4);
        if (mode) return E >= m ? q : 0.0;
        const double t = 1.0 - fabs(E - m) / dE;
        return (m >= g_lo && m <= g_hi && t > 0.0) ? q * t / dE : 0.0;
    }
    if (E <= e1) return 0.0;
    if (E >= e4) return mode ? q : 0.0;
    if (E < e2) {
        const double a = E - e1, f2 = a / (e2 - e1), f3 = a / (e3 - e1), f4 = a / (e4 - e1);
        const double fr = r == 1 ? f2 : r == 2 ? f3 : f4, pre = mode ? q * f2 * f3 * f4 : v * f2 * f3 / (e4 - e1);
        return r == 0 ? pre * ((mode ? 4.0 : 3.0) - (f2 + f3 + f4)) : pre * fr;
    }
    if (E >= e3) {
        const double d = e4 - E, h1 = d / (e4 - e1), h2 = d / (e4 - e2), h3 = d / (e4 - e3);
        const double hr = r == 0 ? h1 : r == 1 ? h2 : h3, pre = mode ? q * h1 * h2 * h3 : v * h1 * h2 / (e4 - e3);
        const double x = r == 3 ? pre * ((mode ? 4.0 : 3.0) - (h1 + h2 + h3)) : pre * hr;
        return mode ? q - x : x;
    }
    const double a = E - e1, b = E - e2, c = e3 - E, d = e4 - E;
    const double i31 = 1.0 / (e3 - e1), i41 = 1.0 / (e4 - e1), i32 = 1.0 / (e3 - e2), i42 = 1.0 / (e4 - e2);
    const double C1 = q * a * a * i41 * i31, C2 = q * a * b * c * i41 * i32 * i31, C3 = q * b * b * d * i42 * i32 * i41;
    if (mode) {
        return r == 0 ? C1 + (C1 + C2) * c * i31 + (C1 + C2 + C3) * d * i41
             : r == 1 ? C1 + C2 + C3 + (C2 + C3) * c * i32 + C3 * d * i42
             : r == 2 ? (C1 + C2) * a * i31 + (C2 + C3) * b * i32
                      : (C1 + C2 + C3) * a * i41 + C3 * b * i42;
    }
    const double D1 = 2.0 * q * a * i41 * i31, D2 = q * (b * c + a * c - a * b) * i41 * i32 * i31, D3 = q * (2.0 * b * d - b * b) * i42 * i32 * i41;
    return r == 0 ? D1 + ((D1 + D2) * c - (C1 + C2)) * i31 + ((D1 + D2 + D3) * d - (C1 + C2 + C3)) * i41
         : r == 1 ? D1 + D2 + D3 + ((D2 + D3) * c - (C2 + C3)) * i32 + (D3 * d - C3) * i42
         : r == 2 ? ((D1 + D2) * a + (C1 + C2)) * i31 + ((D2 + D3) * b + (C2 + C3)) * i32
                  : ((D1 + D2 + D3) * a + (C1 + C2 + C3)) * i41 + (D3 * b + C3) * i42;
}

// The tile, the W loads, the tails and the epilogue are the DOS tile's (above), and the GEMM runs over the states s = (band, k).  eps ascends
// in b at every k, so band_lo (min over k) and band_hi (max over k) both ascend in b and the bands that matter to the tile are a contiguous range found
// by binary search: DOS -- band_hi >= E_first - 2 dE and band_lo <= E_last + 2 dE (a tetrahedron contributes inside [e1, e4], a flat one within dE of
// its mean; the second dE keeps a rounding of the limit out of the decision); number of states -- band_lo <= E_last, and the bands with band_hi <=
// E_first are full at every energy of the tile: their element is q * (entries of the k-row) without a look at the eigenvalues.  The states of the range,
// (b - b_lo) nk + k, are cut into steps of 4 (one v_mfma_f32_16x16x4_f32 each; a step may straddle two bands) dealt to the 4 waves in contiguous
// quarters.  Per step a lane generates ONE element A[energy lane & 15][state lane >> 4]: it walks the corner table of its k-row in the table's order
// (ascending tetrahedron: the fixed summation order), per entry loads the tetrahedron's four eigenvalues of band b, sorts them (5 comparators), takes
// the rank of its own corner (ties: the lower slot first, so repeated corners of a folded or n_i = 1 grid take distinct ranks) and adds tetra_corner
// in double; the sum is rounded to fp32 once.  The 16 lanes of a state walk the same entries: their loads are one address.  Table entries are clamped
// into range before they index anything.
template <bool VEC>
__global__ __launch_bounds__(64 * DB_WAVES) void dos_tetra_kernel(const float* __restrict__ eps, const float* __restrict__ W, int nk, int nb, int Gp,
                                                                  const int4* __restrict__ tet, int nt, const int32_t* __restrict__ kt_ptr,
                                                                  const int32_t* __restrict__ kt_tet, const int32_t* __restrict__ kt_corner,
                                                                  const float* __restrict__ band_lo, const float* __restrict__ band_hi, double E0,
                                                                  double dE, int ne, int mode, int accumulate, float* __restrict__ D) {
    const DosTile tl = dos_tile<VEC>(Gp);
    const int lane = tl.lane, kq = tl.kq, j0 = tl.j0;
    const int jl = j0 + 15 < ne ? j0 + 15 : ne - 1;
    auto energy = [&](int j) { return __dadd_rn(E0, __dmul_rn((double)j, dE)); };      // (two roundings, as the host computes the grid: no fma)
    const double E_first = energy(j0), E_last = energy(jl), g_lo = E0, g_hi = energy(ne - 1);
    auto first_above = [&](const float* __restrict__ x, double lim, bool strict) {      // first b with x[b] > lim (strict) / >= lim
        int a = 0, b = nb;
        while (a < b) {
            const int m = (a + b) >> 1;
            if (strict ? (double)x[m] <= lim : (double)x[m] < lim) a = m + 1; else b = m;
        }
        return a;
    };
    const int b_lo = mode ? 0 : first_above(band_hi, E_first - 2.0 * dE, false);
    const int b_hi = first_above(band_lo, mode ? E_last : E_last + 2.0 * dE, true);
    const int b_full = mode ? first_above(band_hi, E_first, true) : 0;                   // bands below it: band_hi <= E_first
    const int ns = b_hi > b_lo ? (b_hi - b_lo) * nk : 0;                                 // (the host keeps nk nb below 2^31)
    const int nsteps = (ns + 3) >> 2;
    if (nsteps == 0 && accumulate) return;                     // (block-uniform) no band in reach leaves D alone
    int st0, st1;
    dos_wave_steps(tl, nsteps, st0, st1);
    const double Ej = energy(j0 + tl.sl), v = 1.0 / (double)nt;
    f32x4 acc[DB_NT] = {};
    for (int st = st0; st < st1; ++st) {                       // (wave-uniform bounds; st0 < st1 implies ns > 0)
        const int s_raw = 4 * st + kq, s = s_raw < ns ? s_raw : ns - 1;
        const int bb = s / nk, k = s - bb * nk, b = b_lo + bb;
        float bv[DB_NT];
        dos_load_w<VEC>(W + ((int64_t)k * nb + b) * Gp, tl, Gp, bv);
        const int q0 = kt_ptr[k] > 0 ? kt_ptr[k] : 0, q1 = kt_ptr[k + 1] < 4 * nt ? kt_ptr[k + 1] : 4 * nt;
        double A = 0.0;
        if (b < b_full) {
            A = (double)(q1 - q0) * (0.25 * v);
        } else {
            for (int q = q0; q < q1; ++q) {
                const int slot = kt_corner[q] & 3;
                const int4 cn = tet[hg_clampi(kt_tet[q], nt)];
                auto ev = [&](int kk) { return (double)eps[(int64_t)hg_clampi(kk, nk) * nb + b]; };
                double x0 = ev(cn.x), x1 = ev(cn.y), x2 = ev(cn.z), x3 = ev(cn.w);
                const double me = slot == 0 ? x0 : slot == 1 ? x1 : slot == 2 ? x2 : x3;
                const int r = (int)(x0 < me || (x0 == me && 0 < slot)) + (int)(x1 < me || (x1 == me && 1 < slot)) +
                              (int)(x2 < me || (x2 == me && 2 < slot)) + (int)(x3 < me);
                double t;
#define HG_CSWAP(p, q_) t = fmin(p, q_), q_ = fmax(p, q_), p = t
                HG_CSWAP(x0, x1); HG_CSWAP(x2, x3); HG_CSWAP(x0, x2); HG_CSWAP(x1, x3); HG_CSWAP(x1, x2);
#undef HG_CSWAP
                A += tetra_corner(x0, x1, x2, x3, r, Ej, v, mode, dE, g_lo, g_hi);
            }
        }
        const float av = s_raw < ns ? (float)A : 0.f;
#pragma unroll
        for (int t = 0; t < DB_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
    }
    dos_epilogue<VEC>(acc, tl, ne, Gp, accumulate, D);
}

extern "C" int hg_dos_tetra(const float* eps, const float* W, int nk, int nb, int Gp, const int32_t* tet, int64_t nt, const int32_t* kt_ptr,
                            const int32_t* kt_tet, const int32_t* kt_corner, const float* band_lo, const float* band_hi, double E0, double dE, int ne,
                            int mode, int accumulate, float* D, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ne <= 0) return 0;
    if (!(dE > 0.0) || (mode != 0 && mode != 1) || nt < 0 || nt > 2147483647LL / 4 || Gp < 1 || nk < 0 || nb < 0 ||
        (int64_t)nk * nb > 2147483647LL - 8)
        return hg_fail(-2, "hg_dos_tetra: bad arguments (dE must be positive, mode 0 or 1, nt >= 0, Gp >= 1, nk nb < 2^31)");
    const bool states = nk > 0 && nb > 0 && nt > 0;            // without states every element of D is 0 (or left alone)
    if (!D || (states && (!eps || !W || !tet || !kt_ptr || !kt_tet || !kt_corner || !band_lo || !band_hi)))
        return hg_fail(-2, "hg_dos_tetra: null pointer");
    if ((((uintptr_t)W | (uintptr_t)D | (uintptr_t)tet) & 15)) return hg_fail(-2, "hg_dos_tetra: W, D and tet must be 16-byte aligned");
    dim3 grid;
    if (!dos_grid(ne, Gp, grid)) return hg_fail(-2, "hg_dos_tetra: too many group columns");
    const int nbe = states ? nb : 0;                           // no band in reach of any tile: zeros written / D left alone, nothing read
    HG_DOS_LAUNCH(dos_tetra_kernel, Gp, grid, stream, eps, W, nk, nbe, Gp, (const int4*)tet, (int)nt, kt_ptr, kt_tet, kt_corner, band_lo, band_hi, E0, dE, ne, mode,
                  accumulate ? 1 : 0, D);
    return hg_check_launch("hg_dos_tetra");
}

// ------------------------------------------------------------------------------------------------ kernels on rows of eigenvectors
// launch of kernel_<NT> (256 threads), NT = the 16-orbital tiles that cover nao <= 48
#define HG_NT_LAUNCH(kernel_, nao_, grid_, stream_, ...)                                                  \
    do {                                                                                                  \
        if ((nao_) <= 16) kernel_<1><<<grid_, 256, 0, (hipStream_t)(stream_)>>>(__VA_ARGS__);             \
        else if ((nao_) <= 32) kernel_<2><<<grid_, 256, 0, (hipStream_t)(stream_)>>>(__VA_ARGS__);        \
        else kernel_<3><<<grid_, 256, 0, (hipStream_t)(stream_)>>>(__VA_ARGS__);                          \
    } while (0)

// ------------------------------------------------------------------------------------------------ bond-resolved weights (COOP / COHP)
// The contraction of one member (an edge or an on-site block) that bond_weights_kernel and kgrad_elements_kernel share, for the wave's 16 columns (column
// lane & 15 = one pair of rows (cb, ck) of C; the same row twice for a bond weight): (pr, pi) = sum_{a, b} conj(cb[oi + ri[a]]) X[a][b] ck[oj + rj[b]].  T = X C_ket as two real GEMMs (X times Re and Im) on
// v_mfma_f32_16x16x4_f32 over the nao x nao block as it lies in the row: row tiles of 16 orbitals a (NT of them, 2 NT independent accumulators), steps of 4
// orbitals b; lane l holds A[a = 16 t + (l & 15)][b = 4 step + (l >> 4)] = X[a][b] and B[b][column l & 15].  Orbitals an atom does not have (rank < 0) and the
// tails past nao go by predication: their A and B elements are 0 and nothing is read for them (the load is redirected to element 0 and its value dropped).
// Then per lane sum_a conj(C_bra[a]) T[a] over its rows a = 16 t + 4 (l >> 4) + r (C/D map of the tile), and two shuffles add the four lane quarters: every
// lane of a column ends with the column's sum.  Wave-uniform control flow: every lane reaches every MFMA and shuffle.
template <int NT>
__device__ __forceinline__ void member_contract(const float* __restrict__ X, const int32_t* __restrict__ ri, const int32_t* __restrict__ rj, int oi, int oj,
                                                const float2* __restrict__ cb, const float2* __restrict__ ck, int nao, int M, int sl, int kq, float& pr_out,
                                                float& pi_out) {
    int ra[NT];                                            // rank of this lane's A row a = 16 t + sl, or -1
    f32x4 tr[NT], ti[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int a = 16 * t + sl;
        ra[t] = ri[a < nao ? a : 0];
        ra[t] = a < nao ? ra[t] : -1;
        tr[t] = f32x4{0.f, 0.f, 0.f, 0.f}, ti[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int b0 = 0; b0 < nao; b0 += 4) {
        const int b = b0 + kq;
        int rb = rj[b < nao ? b : 0];
        rb = b < nao ? rb : -1;
        float2 cj = ck[hg_clampi(oj + rb, M)];
        cj = rb >= 0 ? cj : make_float2(0.f, 0.f);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool ok = ra[t] >= 0 && rb >= 0;
            float x = X[ok ? (16 * t + sl) * nao + b : 0];
            x = ok ? x : 0.f;
            tr[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, cj.x, tr[t], 0, 0, 0);
            ti[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, cj.y, ti[t], 0, 0, 0);
        }
    }
    float pr = 0.f, pi = 0.f;                              // sum_a conj(c_bra[a]) T[a] over this lane's rows: C/D map row = 4 (lane >> 4) + r, column of the wave
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = 16 * t + 4 * kq + r;
            int rr = ri[a < nao ? a : 0];
            rr = a < nao ? rr : -1;
            float2 ci = cb[hg_clampi(oi + rr, M)];
            ci = rr >= 0 ? ci : make_float2(0.f, 0.f);
            pr = fmaf(ci.y, ti[t][r], fmaf(ci.x, tr[t][r], pr));
            pi = fmaf(-ci.y, tr[t][r], fmaf(ci.x, ti[t][r], pi));
        }
    pr += __shfl_xor(pr, 16, 64), pi += __shfl_xor(pi, 16, 64);
    pr += __shfl_xor(pr, 32, 64), pi += __shfl_xor(pi, 32, 64);
    pr_out = pr, pi_out = pi;
}

// W[s, 1 + g] = wk[s] * (sum_{e in edges(g)} t_e(s) + sum_{i in atoms(g)} o_i(s)),  t_e(s) = Re(exp(2 pi i k_s . shift_e) c_i^+ X_off[e] c_j), o_i(s) =
// Re(c_i^+ X_on[i] c_i), (i, j) = (erow[e], ecol[e]) the row and column atom of hg_hk_assemble, c_i the entries ooff[i] + orank[i][a] of row s of C.
// One workgroup owns one (tile of 16 states, group); the group's members -- its edges in the order of eidx, then its atoms in the order of aidx -- are
// dealt to the 4 waves in contiguous quarters.  Per member a wave forms c_i^+ X c_j for its 16 states with member_contract (above: two real GEMMs on
// v_mfma_f32_16x16x4_f32 over the nao x nao block as it lies in the row, missing orbitals and tails by predication, so rectangular blocks need no padded
// input), the phase (hg_edge_phase) turns the
// complex sum into t_e, and the member is added to the wave's running sum.  The waves' sums are added through LDS as ((w0 + w1) + w2) + w3: one owner per
// output element, a fixed order, no atomics.  The extra workgroups g = G write column 0 (= wk) and the pad columns (= 0); an empty group writes 0.  A state
// row past ns repeats row ns - 1 and is not stored; the phase is per state, so the states of a tile may belong to different k-points, and a row of W does
// not depend on which other states the launch holds.  Every table entry is clamped into range before it indexes anything.
template <int NT>
__global__ __launch_bounds__(256) void bond_weights_kernel(const float2* __restrict__ Cm, int ns, int M, const int32_t* __restrict__ kidx,
                                                           const float* __restrict__ kvec, int nk, const float* __restrict__ X_on,
                                                           const float* __restrict__ X_off, const int32_t* __restrict__ erow,
                                                           const int32_t* __restrict__ ecol, const float* __restrict__ shift, int E, int n_atoms, int nao,
                                                           const int32_t* __restrict__ orank, const int32_t* __restrict__ ooff,
                                                           const int32_t* __restrict__ eptr, const int32_t* __restrict__ eidx,
                                                           const int32_t* __restrict__ aptr, const int32_t* __restrict__ aidx, int G, int Gp, int ntile,
                                                           const float* __restrict__ wk, float* __restrict__ W) {
    __shared__ float part[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x / ntile, s0 = 16 * (blockIdx.x - g * ntile);
    if (g == G) {                                              // (block-uniform) column 0 and the pad columns 1 + G .. Gp - 1 of the tile's rows
        const int nc = Gp - G;
        for (int q = threadIdx.x; q < 16 * nc; q += 256) {
            const int r = q / nc, c = q - r * nc, s = s0 + r;
            if (s < ns) W[(int64_t)s * Gp + (c == 0 ? 0 : G + c)] = c == 0 ? wk[s] : 0.f;
        }
        return;
    }
    const int sl = lane & 15, kq = lane >> 4;
    const int sc = s0 + sl < ns ? s0 + sl : ns - 1;
    const float2* __restrict__ c = Cm + (int64_t)sc * M;
    const int kp = hg_clampi(kidx[sc], nk);
    const double kx = kvec[3 * kp], ky = kvec[3 * kp + 1], kz = kvec[3 * kp + 2];
    const int e0 = eptr[g], a0 = aptr[g];
    const int ne = E > 0 && eptr[g + 1] > e0 ? eptr[g + 1] - e0 : 0, na = aptr[g + 1] > a0 ? aptr[g + 1] - a0 : 0;
    const int nm = ne + na, chunk = (nm + 3) >> 2;
    const int m0 = wave * chunk, m1 = m0 + chunk < nm ? m0 + chunk : nm;
    const int nao2 = nao * nao;
    float sum = 0.f;
    for (int m = m0; m < m1; ++m) {                            // (wave-uniform bounds and member: every lane reaches every MFMA and shuffle)
        const bool edge = m < ne;
        int i, j;
        const float* __restrict__ X;
        float2 ph = make_float2(1.f, 0.f);
        if (edge) {
            const int e = hg_clampi(eidx[e0 + m], E);
            i = hg_clampi(erow[e], n_atoms), j = hg_clampi(ecol[e], n_atoms);
            X = X_off + (int64_t)e * nao2;
            ph = hg_edge_phase(kx, ky, kz, shift[3 * (int64_t)e], shift[3 * (int64_t)e + 1], shift[3 * (int64_t)e + 2]);
        } else {
            i = j = hg_clampi(aidx[a0 + (m - ne)], n_atoms);
            X = X_on + (int64_t)i * nao2;
        }
        const int32_t* __restrict__ ri = orank + (int64_t)i * nao;
        const int32_t* __restrict__ rj = orank + (int64_t)j * nao;
        const int oi = ooff[i], oj = ooff[j];
        float pr, pi;
        member_contract<NT>(X, ri, rj, oi, oj, c, c, nao, M, sl, kq, pr, pi);
        sum += fmaf(ph.x, pr, -(ph.y * pi));                     // Re(phase * sum); an on-site member has phase 1
    }
    if (kq == 0) part[wave][sl] = sum;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int s = s0 + (int)threadIdx.x;
        if (s < ns) W[(int64_t)s * Gp + 1 + g] = wk[s] * (((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x]);
    }
}

extern "C" int hg_bond_weights(const float* C, int64_t ns, int M, const int32_t* kidx, const float* kvec, int nk, const float* X_on, const float* X_off,
                               const int32_t* erow, const int32_t* ecol, const float* shift, int64_t n_edges, int n_atoms, int nao, const int32_t* orank,
                               const int32_t* ooff, const int32_t* eptr, const int32_t* eidx, const int32_t* aptr, const int32_t* aidx, int G, int Gp,
                               const float* wk, float* W, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ns <= 0) return 0;
    const int64_t ntile = (ns + 15) / 16;
    if (M <= 0 || nk <= 0 || n_atoms <= 0 || nao <= 0 || nao > 48 || n_edges < 0 || n_edges > 2147483647LL || G < 0 || Gp < 1 + G || ns > 2147483647LL - 16 ||
        ntile * ((int64_t)G + 1) > 2147483647LL)
        return hg_fail(-2, "hg_bond_weights: bad sizes (M, nk, n_atoms >= 1, 1 <= nao <= 48, Gp >= 1 + G, ceil(ns / 16) (G + 1) < 2^31)");
    if (!C || !kidx || !kvec || !X_on || !orank || !ooff || !eptr || !aptr || !wk || !W || (n_edges > 0 && (!X_off || !erow || !ecol || !shift)))
        return hg_fail(-2, "hg_bond_weights: null pointer");
    const dim3 grid((unsigned)(ntile * ((int64_t)G + 1)));
    HG_NT_LAUNCH(bond_weights_kernel, nao, grid, stream, (const float2*)C, (int)ns, M, kidx, kvec, nk, X_on, X_off, erow, ecol, shift, (int)n_edges, n_atoms, nao, orank, ooff,
                 eptr, eidx, aptr, aidx, G, Gp, (int)ntile, wk, W);
    return hg_check_launch("hg_bond_weights");
}

// ------------------------------------------------------------------------------------------------ density-matrix rows
// P_off[e][a, b] (+)= sum_s f_s Re(exp(2 pi i k_s . shift_e) conj(C[s][mu(i, a)]) C[s][mu(j, b)]),  P_on[i][a, b] the same with j = i and no phase; (i, j) =
// (erow[e], ecol[e]) and mu(i, a) = ooff[i] + orank[i][a] as above.  A sampled dense-dense product (SDDMM): per member (an edge or an atom) an n_i x n_j
// block with K = the states.  One workgroup owns one member (blocks 0 .. E - 1 the edges, E .. E + n_atoms - 1 the atoms); the steps of 4 states (one
// v_mfma_f32_16x16x4_f32 each) are dealt to the 4 waves in contiguous quarters.  The block is tiled over the COMPACT ranks r = orank[i][a] (tiles of 16, NT x NT
// accumulators): lane l holds A[r_a = 16 t + (l & 15)][state l >> 4] = f_s (x, y) of C[s][ooff[i] + r_a] and B[state l >> 4][r_b = 16 t + (l & 15)] =
// (x', y') = exp(i theta) C[s][ooff[j] + r_b] -- the column operand is rotated once per loaded element, so that Re(phase conj(c_a) c_b) = x_a x'_b + y_a y'_b is
// two real MFMA chains per tile instead of four; 16 lanes read 128 contiguous bytes of a row of C.  cos / sin of theta = 2 pi k . shift are formed once per
// (k-point, member) in a prologue (hg_edge_phase) into a table in LDS of the first DR_KCAP k-points; a
// state whose k-point lies beyond the table forms its own (the slow path of a very large k-list).  Ranks past n_i / n_j and state slots past ns contribute
// operands of 0 (their loads are redirected into range).  The waves' partial tiles go to LDS; the epilogue walks the nao x nao row as it lies in memory
// (coalesced), maps (a, b) to its ranks and adds the four partials as ((w0 + w1) + w2) + w3: one owner per element, a fixed order, no atomics.  accumulate
// 0: every element of the row is written, 0 where an atom lacks the orbital; 1: added to what is there, missing-orbital elements untouched.  A member's
// block does not depend on the other members of the launch.  Every table entry is clamped into range before it indexes anything.
#define DR_KCAP 1024                                         // k-points whose phase of the member is tabulated in LDS (8 KiB)
template <int NT>
__global__ __launch_bounds__(256) void density_rows_kernel(const float2* __restrict__ Cm, int ns, int M, const int32_t* __restrict__ kidx,
                                                           const float* __restrict__ kvec, int nk, const float* __restrict__ f,
                                                           const int32_t* __restrict__ erow, const int32_t* __restrict__ ecol,
                                                           const float* __restrict__ shift, int E, int n_atoms, int nao,
                                                           const int32_t* __restrict__ orank, const int32_t* __restrict__ ooff, int accumulate,
                                                           float* __restrict__ P_on, float* __restrict__ P_off) {
    __shared__ float part[4][NT * NT][4][64];
    __shared__ float2 ptab[DR_KCAP];
    __shared__ int rki[48], rkj[48];                           // rank of orbital a of the row / column atom, or -1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sl = lane & 15, kq = lane >> 4;
    const bool edge = (int)blockIdx.x < E;                     // (block-uniform)
    int i, j;
    float* __restrict__ out;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (edge) {
        const int64_t e = blockIdx.x;
        i = hg_clampi(erow[e], n_atoms), j = hg_clampi(ecol[e], n_atoms);
        out = P_off + e * nao * nao;
        sx = shift[3 * e], sy = shift[3 * e + 1], sz = shift[3 * e + 2];
    } else {
        i = j = (int)blockIdx.x - E;
        out = P_on + (int64_t)i * nao * nao;
    }
    auto phase = [&](int kp) { return hg_edge_phase(kvec[3 * kp], kvec[3 * kp + 1], kvec[3 * kp + 2], sx, sy, sz); };
    if ((int)threadIdx.x < nao) {
        const int a = threadIdx.x, ra = orank[(int64_t)i * nao + a], rb = orank[(int64_t)j * nao + a];
        rki[a] = ra >= 0 && ra < 16 * NT ? ra : -1;
        rkj[a] = rb >= 0 && rb < 16 * NT ? rb : -1;
    }
    if (edge)
        for (int kp = threadIdx.x; kp < nk && kp < DR_KCAP; kp += 256) ptab[kp] = phase(kp);
    __syncthreads();
    int ni = 0, nj = 0;                                        // orbitals the two atoms have: the ranks 0 .. n - 1 of a well-formed table
    for (int a = 0; a < nao; ++a) ni += rki[a] >= 0, nj += rkj[a] >= 0;
    const int oi = ooff[i], oj = ooff[j];
    bool va[NT], vb[NT];
    int ca[NT], cb[NT];                                        // this lane's columns of C: rank 16 t + sl of the row atom (A operand) and of the column atom (B)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        va[t] = 16 * t + sl < ni, vb[t] = 16 * t + sl < nj;
        ca[t] = hg_clampi(oi + (va[t] ? 16 * t + sl : 0), M), cb[t] = hg_clampi(oj + (vb[t] ? 16 * t + sl : 0), M);
    }
    const int nsteps = (ns + 3) >> 2, chunk = (nsteps + 3) >> 2;
    const int st0 = wave * chunk, st1 = st0 + chunk < nsteps ? st0 + chunk : nsteps;
    f32x4 acc[NT][NT];
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) acc[ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one step = this lane's state s = 4 st + kq: its weight, its phase and its 2 NT elements of C.  No branch around a load: a slot past ns reads state
    // ns - 1 with weight 0, a rank past n_i / n_j reads the atom's first orbital and its operand is set to 0.
    auto load = [&](int st, float& fs, float2& ph, float2 (&xa)[NT], float2 (&xb)[NT]) {
        const int s_raw = 4 * st + kq, s = s_raw < ns ? s_raw : ns - 1;
        fs = s_raw < ns ? f[s] : 0.f;
        const float2* __restrict__ c = Cm + (int64_t)s * M;
#pragma unroll
        for (int t = 0; t < NT; ++t) xa[t] = c[ca[t]], xb[t] = c[cb[t]];
        ph = make_float2(1.f, 0.f);
        if (edge) {
            const int kp = hg_clampi(kidx[s], nk);
            if (kp < DR_KCAP) ph = ptab[kp]; else ph = phase(kp);
        }
    };
    auto step = [&](float fs, float2 ph, const float2 (&xa)[NT], const float2 (&xb)[NT]) {
        float ax[NT], ay[NT], bx[NT], by[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            ax[t] = va[t] ? fs * xa[t].x : 0.f, ay[t] = va[t] ? fs * xa[t].y : 0.f;
            const float rx = edge ? fmaf(ph.x, xb[t].x, -(ph.y * xb[t].y)) : xb[t].x;      // exp(i theta) (x + i y); an on-site member has no phase
            const float ry = edge ? fmaf(ph.y, xb[t].x, ph.x * xb[t].y) : xb[t].y;
            bx[t] = vb[t] ? rx : 0.f, by[t] = vb[t] ? ry : 0.f;
        }
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[ta], bx[tb], acc[ta][tb], 0, 0, 0);
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ay[ta], by[tb], acc[ta][tb], 0, 0, 0);
    };
    int st = st0;                                              // (wave-uniform bounds: every lane reaches every MFMA)
    for (; st + 4 <= st1; st += 4) {                           // blocks of 4 steps: all loads of the block are requested before its first MFMA
        float fs[4];
        float2 ph[4], xa[4][NT], xb[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) load(st + u, fs[u], ph[u], xa[u], xb[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) step(fs[u], ph[u], xa[u], xb[u]);
    }
    for (; st < st1; ++st) {
        float fs;
        float2 ph, xa[NT], xb[NT];
        load(st, fs, ph, xa, xb);
        step(fs, ph, xa, xb);
    }
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave][ta * NT + tb][r][lane] = acc[ta][tb][r];
    __syncthreads();
    // C/D map of a 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + r.  Element (a, b) of the row has the ranks (ra, rb): tile (ra >> 4, rb >> 4),
    // register ra & 3, lane 16 ((ra >> 2) & 3) + (rb & 15); consecutive b of an atom are consecutive lanes.
    for (int q = threadIdx.x; q < nao * nao; q += 256) {
        const int a = q / nao, b = q - a * nao, ra = rki[a], rb = rkj[b];
        if (ra >= 0 && rb >= 0) {
            const int t = (ra >> 4) * NT + (rb >> 4), r = ra & 3, ln = 16 * ((ra >> 2) & 3) + (rb & 15);
            const float v = ((part[0][t][r][ln] + part[1][t][r][ln]) + part[2][t][r][ln]) + part[3][t][r][ln];
            out[q] = accumulate ? out[q] + v : v;
        } else if (!accumulate) {
            out[q] = 0.f;
        }
    }
}

extern "C" int hg_density_rows(const float* C, int64_t ns, int M, const int32_t* kidx, const float* kvec, int nk, const float* f, const int32_t* erow,
                               const int32_t* ecol, const float* shift, int64_t n_edges, int n_atoms, int nao, const int32_t* orank, const int32_t* ooff,
                               int accumulate, float* P_on, float* P_off, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (ns < 0) ns = 0;
    if (M <= 0 || nk <= 0 || n_atoms <= 0 || nao <= 0 || nao > 48 || n_edges < 0 || n_edges + (int64_t)n_atoms > 2147483647LL || ns > 2147483647LL - 16)
        return hg_fail(-2, "hg_density_rows: bad sizes (M, nk, n_atoms >= 1, 1 <= nao <= 48, n_edges + n_atoms < 2^31, ns < 2^31 - 16)");
    if (!kvec || !orank || !ooff || !P_on || (ns > 0 && (!C || !kidx || !f)) || (n_edges > 0 && (!erow || !ecol || !shift || !P_off)))
        return hg_fail(-2, "hg_density_rows: null pointer");
    if (ns == 0 && accumulate) return 0;                       // nothing to add; without accumulate the launch writes the zero rows
    const dim3 grid((unsigned)(n_edges + n_atoms));
    HG_NT_LAUNCH(density_rows_kernel, nao, grid, stream, (const float2*)C, (int)ns, M, kidx, kvec, nk, f, erow, ecol, shift, (int)n_edges, n_atoms, nao, orank, ooff,
                 accumulate ? 1 : 0, P_on, P_off);
    return hg_check_launch("hg_density_rows");
}

// ------------------------------------------------------------------------------------------------ k-gradient matrix elements (band velocities)
// out[p, alpha] = sum_e i rvec[e, alpha] exp(2 pi i k_p . shift_e) sum_{a, b} conj(C[bra_p][mu(i, a)]) X_off[e][a, b] C[ket_p][mu(j, b)],  k_p the k-point of
// state ket_p, (i, j) = (erow[e], ecol[e]) and mu(i, a) = ooff[i] + orank[i][a] as above: the element <bra| dX(k)/dk_alpha |ket> of the k-derivative of the
// assembled matrix (its on-site blocks do not depend on k), without the M x M matrix.  The per-edge contraction is member_contract, the one of bond_weights_kernel, with two
// rows of C: T = X C_ket as two real GEMMs on v_mfma_f32_16x16x4_f32 (row tiles of 16 orbitals, steps of 4, tails and missing orbitals by predication),
// conj(C_bra) . T over the lane's rows in the C/D layout, two shuffles, then the phase (hg_edge_phase) as a complex product
// z_e, and per Cartesian component the running sums Re += -rvec z.im, Im += rvec z.re (one fused multiply-add each: a zero column of rvec gives exactly 0).
// The single "group" is all E edges, so the edges are split: one workgroup owns one (tile of 16 pairs, chunk of hg_kgrad_chunk_edges(E) consecutive
// edges); the chunk is dealt to the 4 waves in contiguous quarters, the waves' sums are added through LDS as ((w0 + w1) + w2) + w3 and stored to
// part[chunk][pair][6] (or straight to out when there is one chunk).  kgrad_reduce_kernel then adds the chunks in ascending order: one owner per output
// element, a fixed order, no atomics.  The chunk size depends on E alone, so a pair's bits depend neither on the launch's other pairs nor on their number;
// a launch of one pair still spreads over ceil(E / chunk) workgroups.  A pair slot past n_pairs repeats pair n_pairs - 1 and is not stored.  Every table
// entry (bra, ket, kidx, erow, ecol, orank / ooff) is clamped into range before it indexes anything.
template <int NT>
__global__ __launch_bounds__(256) void kgrad_elements_kernel(const float2* __restrict__ Cm, int ns, int M, const int32_t* __restrict__ bra,
                                                             const int32_t* __restrict__ ket, int n_pairs, const int32_t* __restrict__ kidx,
                                                             const float* __restrict__ kvec, int nk, const float* __restrict__ X_off,
                                                             const int32_t* __restrict__ erow, const int32_t* __restrict__ ecol,
                                                             const float* __restrict__ shift, const float* __restrict__ rvec, int E, int n_atoms, int nao,
                                                             const int32_t* __restrict__ orank, const int32_t* __restrict__ ooff, int ntile, int chunk,
                                                             float* __restrict__ dst) {
    __shared__ float part[4][6][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.x / ntile, p0 = 16 * (blockIdx.x - ch * ntile);
    const int sl = lane & 15, kq = lane >> 4;
    const int pc = p0 + sl < n_pairs ? p0 + sl : n_pairs - 1;
    const int sk = hg_clampi(ket[pc], ns), sb = hg_clampi(bra[pc], ns);
    const float2* __restrict__ ck = Cm + (int64_t)sk * M;
    const float2* __restrict__ cb = Cm + (int64_t)sb * M;
    const int kp = hg_clampi(kidx[sk], nk);
    const double kx = kvec[3 * kp], ky = kvec[3 * kp + 1], kz = kvec[3 * kp + 2];
    const int eb = ch * chunk, ee = eb + chunk < E ? eb + chunk : E;
    const int quarter = (ee - eb + 3) >> 2;
    const int m0 = eb + wave * quarter, m1 = m0 + quarter < ee ? m0 + quarter : ee;
    const int nao2 = nao * nao;
    float ar[3] = {0.f, 0.f, 0.f}, ai[3] = {0.f, 0.f, 0.f};
    for (int e = m0; e < m1; ++e) {                            // (wave-uniform bounds and edge: every lane reaches every MFMA and shuffle)
        const int i = hg_clampi(erow[e], n_atoms), j = hg_clampi(ecol[e], n_atoms);
        const float* __restrict__ X = X_off + (int64_t)e * nao2;
        const float2 ph = hg_edge_phase(kx, ky, kz, shift[3 * (int64_t)e], shift[3 * (int64_t)e + 1], shift[3 * (int64_t)e + 2]);
        const int32_t* __restrict__ ri = orank + (int64_t)i * nao;
        const int32_t* __restrict__ rj = orank + (int64_t)j * nao;
        const int oi = ooff[i], oj = ooff[j];
        float pr, pi;
        member_contract<NT>(X, ri, rj, oi, oj, cb, ck, nao, M, sl, kq, pr, pi);
        const float zr = fmaf(ph.x, pr, -(ph.y * pi)), zi = fmaf(ph.x, pi, ph.y * pr);      // z = phase * sum
#pragma unroll
        for (int al = 0; al < 3; ++al) {                       // i r z = -r z.im + i r z.re
            const float r = rvec[3 * (int64_t)e + al];
            ar[al] = fmaf(-r, zi, ar[al]), ai[al] = fmaf(r, zr, ai[al]);
        }
    }
    if (kq == 0) {
#pragma unroll
        for (int al = 0; al < 3; ++al) part[wave][2 * al][sl] = ar[al], part[wave][2 * al + 1][sl] = ai[al];
    }
    __syncthreads();
    if (threadIdx.x < 96) {                                    // 16 pairs x 6 floats, contiguous in dst
        const int r = (int)threadIdx.x / 6, q = (int)threadIdx.x - 6 * r, p = p0 + r;
        if (p < n_pairs) dst[((int64_t)ch * n_pairs + p) * 6 + q] = ((part[0][q][r] + part[1][q][r]) + part[2][q][r]) + part[3][q][r];
    }
}

// out[x] = sum of part[c][x] over the chunks c in ascending order (x over the 6 n_pairs floats of out); no chunk (E = 0): zeros
__global__ __launch_bounds__(256) void kgrad_reduce_kernel(const float* __restrict__ part, int64_t n, int nchunk, float* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += part[(int64_t)c * n + x];
    out[x] = s;
}

extern "C" int hg_kgrad_elements(const float* C, int64_t ns, int M, const int32_t* bra, const int32_t* ket, int64_t n_pairs, const int32_t* kidx,
                                 const float* kvec, int nk, const float* X_off, const int32_t* erow, const int32_t* ecol, const float* shift,
                                 const float* rvec, int64_t n_edges, int n_atoms, int nao, const int32_t* orank, const int32_t* ooff, float* part,
                                 float* out, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (n_pairs <= 0) return 0;
    const int64_t ntile = (n_pairs + 15) / 16;
    if (ns <= 0 || ns > 2147483647LL || M <= 0 || nk <= 0 || n_atoms <= 0 || nao <= 0 || nao > 48 || n_edges < 0 || n_edges > 1073741824LL ||
        n_pairs > (2147483647LL - 255) / 6 || ntile * hg_kgrad_chunks(n_edges) > 2147483647LL)
        return hg_fail(-2, "hg_kgrad_elements: bad sizes (ns, M, nk, n_atoms >= 1, 1 <= nao <= 48, 0 <= n_edges <= 2^30, 6 n_pairs < 2^31 - 255, ceil(n_pairs / 16) chunks < 2^31)");
    const int nchunk = (int)hg_kgrad_chunks(n_edges);
    if (!C || !bra || !ket || !kidx || !kvec || !orank || !ooff || !out || (n_edges > 0 && (!X_off || !erow || !ecol || !shift || !rvec)) ||
        (nchunk > 1 && !part))
        return hg_fail(-2, "hg_kgrad_elements: null pointer");
    if (nchunk > 0) {
        const dim3 grid((unsigned)(ntile * nchunk));
        float* dst = nchunk > 1 ? part : out;
        HG_NT_LAUNCH(kgrad_elements_kernel, nao, grid, stream, (const float2*)C, (int)ns, M, bra, ket, (int)n_pairs, kidx, kvec, nk, X_off, erow, ecol, shift, rvec, (int)n_edges,
                     n_atoms, nao, orank, ooff, (int)ntile, (int)hg_kgrad_chunk_edges(n_edges), dst);
        if (nchunk == 1) return hg_check_launch("hg_kgrad_elements");
    }
    const int64_t n = 6 * n_pairs;
    kgrad_reduce_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(part, n, nchunk, out);
    return hg_check_launch("hg_kgrad_elements");
}
