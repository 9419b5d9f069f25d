// sym_contraction.hip -- the MACE symmetric contraction of a CorrProductBlock on the nodes (gfx950; reference: hamgnn/nn/interaction_blocks.py:234-260 ->
// toolbox/mace/modules/symmetric_contraction.py).  The three routes of hamgnn_amd/nn.py:CorrProductBlock:
//   hg_sym_contraction                 the nu <= 2 part of every block (correlation 1 ... 4): writes the rows
//   hg_sym_contraction3                the nu = 3 term of correlation 3 and 4, ADDED onto those rows (backward: hamgnn_amd/corr3.py)
//   hg_sym_contraction_nu / _backward  one term of any order nu = 1 ... 4 and its adjoint: the nu = 4 term of correlation 4; every term under HG_CORR_KERNEL=nu
// Hand-written HIP for gfx950 (CDNA4).
#include "hg_device.h"

// ------------------------------------------------------------------------------------------------ nu <= 2
// MACE symmetric contraction with correlation <= 2 on the nodes (hamgnn/nn/interaction_blocks.py:234-260 ->
// toolbox/mace/modules/symmetric_contraction.py:212-230), sparse form of the reference's dense einsums:
//   out[o, c] = sum_x ( sum_(e in row1(o)) U1 W1[z, kap, c]  +  sum_(e in row2(o)) U2 W2[z, kap, c] x[c, i] ) x[c, x]
// One workgroup per node; the node's hidden features x[c][ell] sit in LDS; one thread per (output element o, channel c).
// Node-level and off in the shipped configurations: written for correctness and coalesced weight reads, not tuned.
__global__ __launch_bounds__(256) void sym_contraction_kernel(const float* __restrict__ h, int64_t hs, const int64_t* __restrict__ z, int C, int num_ell,
                                                              const int* __restrict__ ell_off, int nout, const int* __restrict__ out_off,
                                                              const int* __restrict__ ptr1, const int4* __restrict__ ent1,
                                                              const int* __restrict__ ptr2, const int4* __restrict__ ent2,
                                                              const float* __restrict__ W1, int K1, const float* __restrict__ W2, int K2,
                                                              float* __restrict__ out, int64_t os) {
    extern __shared__ float xs[];                              // [num_ell][C]
    const int64_t b = blockIdx.x;
    const float* __restrict__ hb = h + b * hs;
    for (int i = threadIdx.x; i < num_ell * C; i += blockDim.x) {
        const int ell = i / C, c = i - ell * C;
        xs[i] = hb[ell_off[ell] + c];
    }
    __syncthreads();
    const int64_t zb = z[b];
    const float* __restrict__ w1 = W1 + zb * (int64_t)K1 * C;
    const float* __restrict__ w2 = W2 + zb * (int64_t)K2 * C;
    for (int idx = threadIdx.x; idx < nout * C; idx += blockDim.x) {
        const int o = idx / C, c = idx - o * C;
        float acc = 0.f;
        for (int e = ptr1[o]; e < ptr1[o + 1]; ++e) {
            const int4 t = ent1[e];                            // {x, kappa, -, value}
            acc = fmaf(__int_as_float(t.w) * w1[t.y * C + c], xs[t.x * C + c], acc);
        }
        for (int e = ptr2[o]; e < ptr2[o + 1]; ++e) {
            const int4 t = ent2[e];                            // {x, i, kappa, value}
            acc = fmaf(__int_as_float(t.w) * w2[t.z * C + c] * xs[t.y * C + c], xs[t.x * C + c], acc);
        }
        out[b * os + out_off[o] + c] = acc;
    }
}

extern "C" int hg_sym_contraction(const float* h, int64_t h_stride, const int64_t* z, int64_t N, int C, int num_ell, const int32_t* ell_off,
                                  int nout, const int32_t* out_off, const int32_t* ptr1, const int32_t* ent1, const int32_t* ptr2,
                                  const int32_t* ent2, const float* W1, int K1, const float* W2, int K2, float* out, int64_t out_stride,
                                  void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (N <= 0) return 0;
    const size_t lds = sizeof(float) * (size_t)num_ell * C;
    if (lds > 64 * 1024) return hg_fail(-2, "hg_sym_contraction: hidden features too wide for the LDS-resident kernel");
    sym_contraction_kernel<<<dim3((unsigned)N), 256, lds, (hipStream_t)stream>>>(h, h_stride, z, C, num_ell, ell_off, nout, out_off, ptr1,
                                                                                 (const int4*)ent1, ptr2, (const int4*)ent2, W1, K1, W2, K2, out,
                                                                                 out_stride);
    return hg_check_launch("hg_sym_contraction");
}

// ------------------------------------------------------------------------------------------------ nu = 3
// The nu = 3 term of the MACE symmetric contraction of a CorrProductBlock built with `correlation: 3`
// (hamgnn/nn/interaction_blocks.py:234-260 -> toolbox/mace/modules/symmetric_contraction.py:148-230: the main einsum
// "[w] x v i k, ekc, bci, be -> bc [w] x v" whose two open component indices the following nu = 2 / nu = 1 steps contract with x again;
// U_matrix_real of toolbox/mace/tools/cg.py:16-131 for three factors).  ADDED onto the rows that hg_sym_contraction (above) wrote for
// nu <= 2:
//     out[n, o, c] += sum_{(x, i, j, kap, v) in ent3[o]} v W3[z_n, kap, c] h[n, x, c] h[n, i, c] h[n, j, c]
// with U_3 given sparsely by plan.py:sym_contraction_tables (entries in the reference's path order, CSR rows per output element o).
// Node-level and optional (correlation 3 is not the reference's default): one workgroup per node, the node's hidden components in LDS, a lane
// owns one (output element, channel) and walks its entry list in order -- a fixed summation order, no atomics.  HBM traffic per node: its hidden
// row once, its output row read + written once; the entry table (12-100 k entries x 20 B) and the element's weight block stay in L2.
#define C3_ENT_I32 5             // {x, i, j, kappa (global over the targets), value (float bits)}

__global__ __launch_bounds__(256) void sym_contraction3_kernel(const float* __restrict__ h, int64_t hs, const int64_t* __restrict__ z, int C, int num_ell,
                                                               const int* __restrict__ ell_off, int nout, const int* __restrict__ out_off,
                                                               const int* __restrict__ ptr3, const int* __restrict__ ent3,
                                                               const float* __restrict__ W3, int K3, float* __restrict__ out, int64_t os) {
    extern __shared__ float xs[];                              // [num_ell][C]
    const int64_t b = blockIdx.x;
    const float* __restrict__ hb = h + b * hs;
    for (int i = threadIdx.x; i < num_ell * C; i += blockDim.x) {
        const int ell = i / C, c = i - ell * C;
        xs[i] = hb[ell_off[ell] + c];
    }
    __syncthreads();
    const float* __restrict__ w3 = W3 + z[b] * (int64_t)K3 * C;
    for (int idx = threadIdx.x; idx < nout * C; idx += blockDim.x) {
        const int o = idx / C, c = idx - o * C;
        float acc = 0.f;
        for (int e = ptr3[o]; e < ptr3[o + 1]; ++e) {
            const int* __restrict__ t = ent3 + (int64_t)e * C3_ENT_I32;
            const float w = __int_as_float(t[4]) * w3[t[3] * C + c];
            acc = fmaf(w * xs[t[0] * C + c] * xs[t[1] * C + c], xs[t[2] * C + c], acc);
        }
        out[b * os + out_off[o] + c] += acc;
    }
}

extern "C" int hg_sym_contraction3(const float* h, int64_t h_stride, const int64_t* z, int64_t N, int C, int num_ell, const int32_t* ell_off,
                                   int nout, const int32_t* out_off, const int32_t* ptr3, const int32_t* ent3, const float* W3, int K3,
                                   float* out, int64_t out_stride, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (N <= 0) return 0;
    if (!h || !z || !ell_off || !out_off || !ptr3 || !ent3 || !W3 || !out) return hg_fail(-1, "hg_sym_contraction3: null pointer");
    const size_t lds = (size_t)num_ell * C * sizeof(float);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_sym_contraction3: hidden features too wide for the LDS-resident kernel");
    sym_contraction3_kernel<<<dim3((unsigned)N), 256, lds, (hipStream_t)stream>>>(h, h_stride, z, C, num_ell, ell_off, nout, out_off, ptr3, ent3, W3, K3,
                                                                                  out, out_stride);
    return hg_check_launch("hg_sym_contraction3");
}

// ------------------------------------------------------------------------------------------------ any order nu = 1 ... 4 and its adjoint
// One term of the MACE symmetric contraction of a CorrProductBlock, generic in the order nu in {1 ... 4}, and its adjoint
// (reference: hamgnn/nn/interaction_blocks.py:234-260 -> toolbox/mace/modules/symmetric_contraction.py:148-230, U_matrix_real of
// toolbox/mace/tools/cg.py:16-131).  Forward, ADDED onto rows that already exist:
//     out[n, o, c] += sum_{e in ent[o]} v_e W[z_n, kap_e, c] prod_{t < nu} x[n, i_{e,t}, c]
// with U_nu given sparsely by plan.sym_contraction_tables (CSR rows per output element o; a row of `ent` is {i_0 .. i_{nu-1}, kappa, .., value bits}:
// kappa in column nu, the value in the last of max(4, nu + 2) columns -- the layout ent1 / ent2 / ent3 / ent4 share).
//
// Forward: the shape of sym_contraction3_kernel (above) -- one workgroup per node, the node's hidden components in LDS, CSR rows per output
// element.  At nu = 4 the rows are long and uneven (55 ... 148 paths per target, 10^3 - 10^5 entries per row) and nout * C can be far below the 256
// lanes, so a row is dealt to S lanes (S a power of two chosen from nout * C alone, entry e of the row to lane e mod S); the S partial sums meet in LDS
// and ONE lane adds them in the order 0 ... S-1: a fixed summation order, no atomics.
// Adjoint: g_h[n, i, c] = sum over every (entry, position) whose position reads component i -- the same kernel shape on the table transposed by
// component (plan.sym_contraction_adjoint_tables: row {o, the other nu - 1 components, kappa, value bits}), with the node's gradient row in LDS as well;
// g_W[g, kap, c] = sum over the nodes of group g IN INDEX ORDER and the entries of kappa (table transposed by kappa, rows {planar offset of o, planar
// offsets of the nu components, value bits}): a lane owns one (group, kappa, channel), so every element of g_W is written once, without atomics.  A
// group is an element's node list (or a run of it; the caller adds the runs in order) or, under charge doping, the node itself.
#define SN_THREADS 256

static inline int sn_width(int nu) { return nu + 2 < 4 ? 4 : nu + 2; }

// lanes per CSR row: the largest power of two S with S * items <= 256 (1 when the items fill the workgroup)
static inline int sn_split(int items) {
    int s = 1;
    while (s * 2 * items <= SN_THREADS) s *= 2;
    return s;
}

// rows: CSR over `nrow` row owners (forward: output elements, adjoint: components).  A table row holds NF factor indices starting at column F0, the
// owner-side gradient index in column 0 when WITH_G (adjoint), kappa in column KC, the value in column width - 1.
template <int NF, bool WITH_G>
__global__ __launch_bounds__(SN_THREADS) void sym_nu_rows_kernel(const float* __restrict__ h, int64_t hs, const float* __restrict__ g, int64_t gs,
                                                                 const int64_t* __restrict__ z, int C, int num_ell, const int* __restrict__ ell_off,
                                                                 int nout, const int* __restrict__ out_off, int nrow, const int* __restrict__ row_off,
                                                                 const int* __restrict__ ptr, const int* __restrict__ ent, int width,
                                                                 const float* __restrict__ W, int K, float* __restrict__ dst, int64_t ds, int S) {
    extern __shared__ float sm[];
    float* __restrict__ xs = sm;                               // [num_ell][C]
    float* __restrict__ gx = sm + num_ell * C;                 // [nout][C]    (adjoint only)
    float* __restrict__ part = gx + (WITH_G ? nout * C : 0);   // [SN_THREADS]
    constexpr int F0 = WITH_G ? 1 : 0, KC = F0 + NF;
    const int64_t b = blockIdx.x;
    const float* __restrict__ hb = h + b * hs;
    for (int i = threadIdx.x; i < num_ell * C; i += blockDim.x) {
        const int ell = i / C, c = i - ell * C;
        xs[i] = hb[ell_off[ell] + c];
    }
    if (WITH_G) {
        const float* __restrict__ gb = g + b * gs;
        for (int i = threadIdx.x; i < nout * C; i += blockDim.x) {
            const int o = i / C, c = i - o * C;
            gx[i] = gb[out_off[o] + c];
        }
    }
    __syncthreads();
    const float* __restrict__ w = W + z[b] * (int64_t)K * C;
    const int items = nrow * C, ipp = SN_THREADS / S;          // (row owner, channel) items, items per pass
    const int s = threadIdx.x / ipp, li = threadIdx.x - s * ipp;
    for (int base = 0; base < items; base += ipp) {            // uniform trip count: the barriers below are reached by every lane
        const int item = base + li;
        const bool live = item < items;
        const int r = live ? item / C : 0, c = live ? item - r * C : 0;
        float acc = 0.f;
        if (live) {
            for (int e = ptr[r] + s; e < ptr[r + 1]; e += S) {
                const int* __restrict__ t = ent + (int64_t)e * width;
                float p = __int_as_float(t[width - 1]) * w[t[KC] * C + c];
                if (WITH_G) p *= gx[t[0] * C + c];
#pragma unroll
                for (int f = 0; f < NF; ++f) p *= xs[t[F0 + f] * C + c];
                acc += p;
            }
        }
        if (S == 1) {
            if (live) dst[b * ds + row_off[r] + c] += acc;
        } else {
            part[threadIdx.x] = acc;
            __syncthreads();
            if (s == 0 && live) {
                float sum = part[li];
                for (int q = 1; q < S; ++q) sum += part[q * ipp + li];         // fixed order
                dst[b * ds + row_off[r] + c] += sum;
            }
            __syncthreads();
        }
    }
}

// g_W[grp, kap, c] = sum_{n in group grp, in list order} sum_{e in entW[kap]} v_e g[n, o_e, c] prod_t h[n, i_{e,t}, c]   (offsets resolved by the planner)
template <int NU>
__global__ __launch_bounds__(SN_THREADS) void sym_nu_wgrad_kernel(const float* __restrict__ h, int64_t hs, const float* __restrict__ g, int64_t gs, int C,
                                                                  const int* __restrict__ ptrW, const int* __restrict__ entW, int K,
                                                                  const int* __restrict__ grp_ptr, const int* __restrict__ grp_idx,
                                                                  float* __restrict__ gW) {
    const int kc = blockIdx.y * SN_THREADS + threadIdx.x;
    if (kc >= K * C) return;
    const int kap = kc / C, c = kc - kap * C;
    const int64_t grp = blockIdx.x;
    const int n0 = grp_ptr ? grp_ptr[grp] : (int)grp, n1 = grp_ptr ? grp_ptr[grp + 1] : (int)grp + 1;
    const int e0 = ptrW[kap], e1 = ptrW[kap + 1];
    float acc = 0.f;
    for (int q = n0; q < n1; ++q) {
        const int64_t n = grp_idx ? grp_idx[q] : q;
        const float* __restrict__ hb = h + n * hs + c;
        const float* __restrict__ gb = g + n * gs + c;
        float a = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int* __restrict__ t = entW + (int64_t)e * (NU + 2);
            float p = __int_as_float(t[NU + 1]) * gb[t[0]];
#pragma unroll
            for (int f = 0; f < NU; ++f) p *= hb[t[1 + f]];
            a += p;
        }
        acc += a;
    }
    gW[(grp * K + kap) * C + c] = acc;
}

template <int NF, bool WITH_G>
static int sn_launch_rows(const float* h, int64_t hs, const float* g, int64_t gs, const int64_t* z, int64_t N, int C, int num_ell, const int32_t* ell_off,
                          int nout, const int32_t* out_off, int nrow, const int32_t* row_off, const int32_t* ptr, const int32_t* ent, int width,
                          const float* W, int K, float* dst, int64_t ds, size_t lds, hipStream_t st) {
    sym_nu_rows_kernel<NF, WITH_G><<<dim3((unsigned)N), SN_THREADS, lds, st>>>(h, hs, g, gs, z, C, num_ell, ell_off, nout, out_off, nrow, row_off, ptr, ent,
                                                                                 width, W, K, dst, ds, sn_split(nrow * C));
    return 0;
}

extern "C" int hg_sym_contraction_nu(int nu, const float* h, int64_t h_stride, const int64_t* z, int64_t N, int C, int num_ell, const int32_t* ell_off,
                                     int nout, const int32_t* out_off, const int32_t* ptr, const int32_t* ent, const float* W, int K, float* out,
                                     int64_t out_stride, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (nu < 1 || nu > 4) return hg_fail(-3, "hg_sym_contraction_nu: the order nu must be 1 ... 4");
    if (N <= 0) return 0;
    if (!h || !z || !ell_off || !out_off || !ptr || !ent || !W || !out) return hg_fail(-1, "hg_sym_contraction_nu: null pointer");
    if (C <= 0 || num_ell <= 0 || nout <= 0 || K <= 0) return hg_fail(-1, "hg_sym_contraction_nu: empty shape");
    const size_t lds = ((size_t)num_ell * C + SN_THREADS) * sizeof(float);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_sym_contraction_nu: hidden features too wide for the LDS-resident kernel");
    hipStream_t st = (hipStream_t)stream;
#define SN_FWD(NF) sn_launch_rows<NF, false>(h, h_stride, nullptr, 0, z, N, C, num_ell, ell_off, nout, out_off, nout, out_off, ptr, ent, sn_width(nu), W, K, out, out_stride, lds, st)
    switch (nu) {
        case 1: SN_FWD(1); break;
        case 2: SN_FWD(2); break;
        case 3: SN_FWD(3); break;
        default: SN_FWD(4); break;
    }
#undef SN_FWD
    return hg_check_launch("hg_sym_contraction_nu");
}

extern "C" int hg_sym_contraction_nu_backward(int nu, const float* h, int64_t h_stride, const float* g_out, int64_t g_stride, const int64_t* z, int64_t N,
                                              int C, int num_ell, const int32_t* ell_off, int nout, const int32_t* out_off, const int32_t* ptrH,
                                              const int32_t* entH, const int32_t* ptrW, const int32_t* entW, const float* W, int K, int64_t G,
                                              const int32_t* grp_ptr, const int32_t* grp_idx, float* g_h, int64_t gh_stride, float* g_W, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (nu < 1 || nu > 4) return hg_fail(-3, "hg_sym_contraction_nu_backward: the order nu must be 1 ... 4");
    if (N <= 0 || G <= 0) return 0;
    if (!h || !g_out || !z || !ell_off || !out_off || !ptrH || !entH || !ptrW || !entW || !W || !g_h || !g_W)
        return hg_fail(-1, "hg_sym_contraction_nu_backward: null pointer");
    if (C <= 0 || num_ell <= 0 || nout <= 0 || K <= 0) return hg_fail(-1, "hg_sym_contraction_nu_backward: empty shape");
    if (!grp_ptr && G != N) return hg_fail(-1, "hg_sym_contraction_nu_backward: without a group list every node is its own group (G == N)");
    const size_t lds = ((size_t)(num_ell + nout) * C + SN_THREADS) * sizeof(float);
    if (lds > 64 * 1024) return hg_fail(-2, "hg_sym_contraction_nu_backward: hidden features too wide for the LDS-resident kernel");
    hipStream_t st = (hipStream_t)stream;
    const dim3 wg((unsigned)G, (unsigned)(((int64_t)K * C + SN_THREADS - 1) / SN_THREADS));
    // the table by component has one factor less than the order: the position that reads the component is the one differentiated
#define SN_BWD(NU)                                                                                                                                         \
    sn_launch_rows<NU - 1, true>(h, h_stride, g_out, g_stride, z, N, C, num_ell, ell_off, nout, out_off, num_ell, ell_off, ptrH, entH, NU + 2, W, K, g_h,    \
                                 gh_stride, lds, st);                                                                                                      \
    sym_nu_wgrad_kernel<NU><<<wg, SN_THREADS, 0, st>>>(h, h_stride, g_out, g_stride, C, ptrW, entW, K, grp_ptr, grp_idx, g_W)
    switch (nu) {
        case 1: SN_BWD(1); break;
        case 2: SN_BWD(2); break;
        case 3: SN_BWD(3); break;
        default: SN_BWD(4); break;
    }
#undef SN_BWD
    return hg_check_launch("hg_sym_contraction_nu_backward");
}
