// kspace.hip -- H(k) / S(k) assembly of one crystal from the real-space blocks and its adjoint (gfx950): the device side of hamgnn_amd/kspace.py
// (band energies, band-gap and overlap losses).  Replaces the index_put(accumulate=True) assembly of hamgnn_output.py:1776-1905.  spectra.hip (DOS)
// works on what the eigensolver returns for these matrices.
#include "hg_device.h"

// ------------------------------------------------------------------------------------------------ k-space assembly (f4: band energies)
// H(k)[i a, j b] = delta_ij H_on[i][a][b] + sum_{e: i -> j} exp(2 pi i k . nbr_shift_e) H_off[e][a][b]  of ONE crystal, written straight in
// the COMPACT orbital basis (orbitals an element does not have are skipped: the reference builds the nao_max-padded matrix and
// masked_selects it, hamgnn_output.py:1776-1905).  The reference accumulates with index_put(accumulate=True) (atomics); here the edges
// are grouped by atom pair on the host (index plumbing) and one block owns one (pair, k): fixed summation order, no atomics.
//   pair_ptr[npairs+1], pair_edges[]: edges of every (i, j) pair (crystal-local edge ids);  pair_ij[npairs][2];
//   orank[n][nao]: rank of orbital a inside atom i's valid set or -1;  ooff[n]: first compact index of atom i;  M: compact dimension;
//   Hk: [nk][M][M] complex64 (float2), zero-initialised by the caller.
__global__ __launch_bounds__(256) void hk_onsite_kernel(const float* __restrict__ on, int nao, const int* __restrict__ orank,
                                                        const int* __restrict__ ooff, int M, int nk, float2* __restrict__ Hk) {
    const int i = blockIdx.x, k = blockIdx.y;
    const int nao2 = nao * nao;
    for (int q = threadIdx.x; q < nao2; q += blockDim.x) {
        const int a = q / nao, b = q - a * nao;
        const int ra = orank[i * nao + a], rb = orank[i * nao + b];
        if (ra < 0 || rb < 0) continue;
        Hk[((int64_t)k * M + ooff[i] + ra) * M + ooff[i] + rb] = make_float2(on[(int64_t)i * nao2 + q], 0.f);
    }
}

__global__ __launch_bounds__(256) void hk_pairs_kernel(const float* __restrict__ off, const float* __restrict__ shift, const float* __restrict__ kvec,
                                                       const int64_t* __restrict__ pair_ptr, const int64_t* __restrict__ pair_edges,
                                                       const int64_t* __restrict__ pair_ij, int nao, const int* __restrict__ orank,
                                                       const int* __restrict__ ooff, int M, float2* __restrict__ Hk) {
    const int64_t p = blockIdx.x;
    const int k = blockIdx.y;
    const int nao2 = nao * nao;
    const int64_t i = pair_ij[2 * p], j = pair_ij[2 * p + 1];
    const int64_t q0 = pair_ptr[p], q1 = pair_ptr[p + 1];
    const float kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    for (int q = threadIdx.x; q < nao2; q += blockDim.x) {
        const int a = q / nao, b = q - a * nao;
        const int ra = orank[i * nao + a], rb = orank[j * nao + b];
        if (ra < 0 || rb < 0) continue;
        float re = 0.f, im = 0.f;
        for (int64_t t = q0; t < q1; ++t) {
            const int64_t e = pair_edges[t];
            const float2 cs = hg_edge_phase(kx, ky, kz, shift[3 * e], shift[3 * e + 1], shift[3 * e + 2]);
            const float h = off[e * nao2 + q];
            re = fmaf(cs.x, h, re);
            im = fmaf(cs.y, h, im);
        }
        float2* dst = Hk + ((int64_t)k * M + ooff[i] + ra) * M + ooff[j] + rb;
        const float2 old = *dst;                               // (i, i) pairs (self images) add onto the on-site block; one owner per element
        *dst = make_float2(old.x + re, old.y + im);
    }
}

extern "C" int hg_hk_assemble(const float* on, const float* off, const float* nbr_shift, const float* kvec, int nk, const int64_t* pair_ptr,
                              const int64_t* pair_edges, const int64_t* pair_ij, int64_t npairs, int n_atoms, int nao, const int32_t* orank,
                              const int32_t* ooff, int M, float* Hk, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (n_atoms <= 0 || nk <= 0 || M <= 0) return 0;
    if (nao <= 0 || nk > 65535) return hg_fail(-2, "hg_hk_assemble: bad sizes");
    hk_onsite_kernel<<<dim3((unsigned)n_atoms, (unsigned)nk), 256, 0, (hipStream_t)stream>>>(on, nao, orank, ooff, M, nk, (float2*)Hk);
    if (npairs > 0)
        hk_pairs_kernel<<<dim3((unsigned)npairs, (unsigned)nk), 256, 0, (hipStream_t)stream>>>(off, nbr_shift, kvec, pair_ptr, pair_edges, pair_ij, nao,
                                                                                             orank, ooff, M, (float2*)Hk);
    return hg_check_launch("hg_hk_assemble");
}

// ------------------------------------------------------------------------------------------------ adjoint of the k-space assembly (band-energy / band-gap losses)
// G [nk][M][M] complex64: gradient of a real loss with respect to H(k) (d/dRe + i d/dIm)  ->
//   g_on[i][a, b]  = sum_k Re G_k[(i a), (i b)]
//   g_off[e][a, b] = sum_k Re(conj(phase_k(e)) G_k[(i a), (j b)]) = sum_k (c G.re + s G.im),   phase_k(e) = exp(2 pi i k . shift_e) = c + i s
// Same pair tables as hk_pairs_kernel.  One workgroup owns one atom pair, one thread one element of the nao^2 block of every edge of the pair:
// ascending k, one fma chain per output element, no atomics.  The (edge, k) phases of HK_ADJ_EC edges x HK_ADJ_KC k-points are computed once per
// workgroup in double (as the forward kernel) and broadcast from LDS; G is read once per chunk of HK_ADJ_EC edges; a thread owns up to HK_ADJ_QP
// elements (q = threadIdx.x + 256 u), so the block is covered in one pass.  Every element of both outputs is
// written (0 where the element lacks an orbital).
#define HK_ADJ_EC 4                                          // edges of a pair per pass over G
#define HK_ADJ_KC 256                                        // k-points per LDS phase chunk
#define HK_ADJ_QP 4                                          // block elements per thread: nao^2 <= 256 * HK_ADJ_QP
__global__ __launch_bounds__(256) void hk_adj_onsite_kernel(const float2* __restrict__ G, int nk, int nao, const int* __restrict__ orank,
                                                            const int* __restrict__ ooff, int M, float* __restrict__ g_on) {
    const int64_t i = blockIdx.x;
    const int nao2 = nao * nao;
    const int64_t oi = ooff[i];
    for (int q = threadIdx.x; q < nao2; q += blockDim.x) {
        const int a = q / nao, b = q - a * nao;
        const int ra = orank[i * nao + a], rb = orank[i * nao + b];
        float acc = 0.f;
        if (ra >= 0 && rb >= 0) {
            const float2* __restrict__ src = G + (oi + ra) * M + oi + rb;
            for (int k = 0; k < nk; ++k) acc += src[(int64_t)k * M * M].x;
        }
        g_on[i * nao2 + q] = acc;
    }
}

__global__ __launch_bounds__(256) void hk_adj_pairs_kernel(const float2* __restrict__ G, const float* __restrict__ shift, const float* __restrict__ kvec,
                                                           int nk, const int64_t* __restrict__ pair_ptr, const int64_t* __restrict__ pair_edges,
                                                           const int64_t* __restrict__ pair_ij, int nao, const int* __restrict__ orank,
                                                           const int* __restrict__ ooff, int M, float* __restrict__ g_off) {
    __shared__ float2 ph[HK_ADJ_EC][HK_ADJ_KC];                // (c, s) of (edge of the chunk, k of the chunk)
    const int64_t p = blockIdx.x;
    const int nao2 = nao * nao;
    const int64_t i = pair_ij[2 * p], j = pair_ij[2 * p + 1];
    const int64_t q0 = pair_ptr[p], q1 = pair_ptr[p + 1];
    const int64_t oi = ooff[i], oj = ooff[j];
    const int64_t MM = (int64_t)M * M;
    int64_t goff[HK_ADJ_QP];                                   // element q = threadIdx.x + 256 u of the block: its offset in G_k, or -1 (orbital absent / q past the block)
#pragma unroll
    for (int u = 0; u < HK_ADJ_QP; ++u) {
        const int q = threadIdx.x + 256 * u;
        goff[u] = -1;
        if (q < nao2) {
            const int a = q / nao, b = q - a * nao;
            const int ra = orank[i * nao + a], rb = orank[j * nao + b];
            if (ra >= 0 && rb >= 0) goff[u] = (oi + ra) * M + oj + rb;
        }
    }
    for (int64_t t0 = q0; t0 < q1; t0 += HK_ADJ_EC) {          // (uniform trip counts: every thread reaches every barrier)
        const int ec = (int)(q1 - t0 < HK_ADJ_EC ? q1 - t0 : HK_ADJ_EC);
        float acc[HK_ADJ_QP][HK_ADJ_EC];
#pragma unroll
        for (int u = 0; u < HK_ADJ_QP; ++u)
#pragma unroll
            for (int x = 0; x < HK_ADJ_EC; ++x) acc[u][x] = 0.f;
        for (int k0 = 0; k0 < nk; k0 += HK_ADJ_KC) {
            const int kc = nk - k0 < HK_ADJ_KC ? nk - k0 : HK_ADJ_KC;
            __syncthreads();                                   // the previous chunk's phases have been read
            if ((int)threadIdx.x < kc) {
                const int k = k0 + threadIdx.x;
                const double kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
                for (int x = 0; x < ec; ++x) {
                    const int64_t e = pair_edges[t0 + x];
                    ph[x][threadIdx.x] = hg_edge_phase(kx, ky, kz, shift[3 * e], shift[3 * e + 1], shift[3 * e + 2]);
                }
            }
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
#pragma unroll
                for (int u = 0; u < HK_ADJ_QP; ++u) {
                    if (goff[u] >= 0) {
                        const float2 gk = G[goff[u] + (int64_t)(k0 + kk) * MM];
#pragma unroll
                        for (int x = 0; x < HK_ADJ_EC; ++x) {
                            if (x < ec) {
                                const float2 cs = ph[x][kk];
                                acc[u][x] = fmaf(cs.y, gk.y, fmaf(cs.x, gk.x, acc[u][x]));
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HK_ADJ_QP; ++u) {
            const int q = threadIdx.x + 256 * u;
            if (q < nao2) {
#pragma unroll
                for (int x = 0; x < HK_ADJ_EC; ++x)
                    if (x < ec) g_off[pair_edges[t0 + x] * nao2 + q] = acc[u][x];   // (0 where the element lacks orbital a or b)
            }
        }
    }
}

extern "C" int hg_hk_assemble_adjoint(const float* G, const float* nbr_shift, const float* kvec, int nk, const int64_t* pair_ptr,
                                      const int64_t* pair_edges, const int64_t* pair_ij, int64_t npairs, int n_atoms, int64_t n_edges, int nao,
                                      const int32_t* orank, const int32_t* ooff, int M, float* g_on, float* g_off, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (n_atoms <= 0 || nk <= 0 || M <= 0) return 0;
    // grid limits of this layout: pairs / atoms on grid.x, nao^2 elements on 256 threads x HK_ADJ_QP; nk is not a grid dimension here, but G is what
    // hg_hk_assemble produced, which takes at most 65535 k-points
    if (nao <= 0 || nao * nao > 256 * HK_ADJ_QP || nk > 65535 || npairs < 0 || npairs > 2147483647LL || npairs > n_edges)
        return hg_fail(-2, "hg_hk_assemble_adjoint: bad sizes");
    hk_adj_onsite_kernel<<<dim3((unsigned)n_atoms), 256, 0, (hipStream_t)stream>>>((const float2*)G, nk, nao, orank, ooff, M, g_on);
    if (npairs > 0)
        hk_adj_pairs_kernel<<<dim3((unsigned)npairs), 256, 0, (hipStream_t)stream>>>((const float2*)G, nbr_shift, kvec, nk, pair_ptr, pair_edges, pair_ij, nao,
                                                                                    orank, ooff, M, g_off);
    return hg_check_launch("hg_hk_assemble_adjoint");
}
