// geometry.hip -- per-edge geometry (gfx950): frame angles, Bessel / Gaussian radial basis and Wigner blocks D^l(R_e) of every edge, and the gather of
// node rows into the edge frame (hamgnn_amd/so3.py is the host twin).  See include/hamgnn_hip.h for the reference op cluster each entry point replaces.
#include "hg_device.h"

// ------------------------------------------------------------------------------------------------ edge geometry
// angles of R_e = Rx(beta) Ry(alpha) taking the e3nn-order unit vector n = (v_y, v_z, v_x)/|v| onto the pole (0,1,0);
// Bessel * cosine-cutoff radial basis evaluated in fp64 (phase n*pi*r/rc by Chebyshev recurrence) and rounded once.
__global__ void geometry_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ei, const float* __restrict__ shift,
                                int64_t E, float cutoff, int R, float4* __restrict__ ang, float* __restrict__ rbf,
                                float* __restrict__ len) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t j = ei[e], i = ei[E + e];
    const double vx = (double)pos[3 * i + 0] + (double)shift[3 * e + 0] - (double)pos[3 * j + 0];
    const double vy = (double)pos[3 * i + 1] + (double)shift[3 * e + 1] - (double)pos[3 * j + 1];
    const double vz = (double)pos[3 * i + 2] + (double)shift[3 * e + 2] - (double)pos[3 * j + 2];
    const double r = sqrt(vx * vx + vy * vy + vz * vz);
    const double inv = r > 0 ? 1.0 / r : 0.0;
    const double nx = vy * inv, ny = vz * inv, nz = vx * inv;            // e3nn axis order = physical (y, z, x)
    const double rho = sqrt(nx * nx + nz * nz);
    double ca = 1.0, sa = 0.0;
    if (rho > 1e-12) { ca = nz / rho; sa = -nx / rho; }
    ang[e] = make_float4((float)ca, (float)sa, (float)ny, (float)(-rho));
    if (len) len[e] = (float)r;
    if (rbf) {
        const double th = M_PI * r / (double)cutoff;
        double s1, c1;
        sincos(th, &s1, &c1);
        const double fc = (r < (double)cutoff) ? 0.5 * (c1 + 1.0) * inv : 0.0;
        double sn = 0.0, cn = 1.0;
        for (int n = 0; n < R; ++n) {
            const double s2 = sn * c1 + cn * s1, c2 = cn * c1 - sn * s1;
            sn = s2; cn = c2;
            rbf[e * R + n] = (float)(sn * fc);
        }
    }
}

// D^l(R_e) = J Z(beta) J^T Z(alpha): one thread per (edge, row a).  (hamgnn_amd/so3.py:edge_wigner is the host twin.)
template <int L>
__device__ __forceinline__ void wigner_rows(const float4* __restrict__ ang, int64_t E, const float* __restrict__ J, const float* __restrict__ sgn,
                                            float* __restrict__ wig, int nW, int off) {
    constexpr int N = 2 * L + 1;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * N) return;
    const int64_t e = idx / N;
    const int a = (int)(idx - e * N);
    const float4 q = ang[e];
    float ca[L + 1], sa[L + 1], cb[L + 1], sb[L + 1];
    ca[0] = cb[0] = 1.f; sa[0] = sb[0] = 0.f;
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        ca[m] = ca[m - 1] * q.x - sa[m - 1] * q.y; sa[m] = sa[m - 1] * q.x + ca[m - 1] * q.y;
        cb[m] = cb[m - 1] * q.z - sb[m - 1] * q.w; sb[m] = sb[m - 1] * q.z + cb[m - 1] * q.w;
    }
    float t1[N], t2[N];
    t1[L] = J[a * N + L];
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        const float jp = J[a * N + L + m], jm = J[a * N + L - m], s = sgn[m] * sb[m];
        t1[L + m] = jp * cb[m] - s * jm;
        t1[L - m] = jm * cb[m] + s * jp;
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int b = 0; b < N; ++b) acc = fmaf(t1[b], J[c * N + b], acc);
        t2[c] = acc;
    }
    float* __restrict__ o = wig + e * nW + off + a * N;
    o[L] = t2[L];
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        const float s = sgn[m] * sa[m];
        o[L + m] = t2[L + m] * ca[m] - s * t2[L - m];
        o[L - m] = t2[L - m] * ca[m] + s * t2[L + m];
    }
}
template <int L>
__global__ void wigner_kernel(const float4* __restrict__ ang, int64_t E, const float* __restrict__ J, const float* __restrict__ sgn,
                              float* __restrict__ wig, int nW, int off) {
    wigner_rows<L>(ang, E, J, sgn, wig, nW, off);
}
// all l in ONE launch (blockIdx.y = l): small crystals, where seven extra launches are 4 % of a forward; blocks past E (2 l + 1) exit
__global__ void wigner_all_kernel(const float4* __restrict__ ang, int64_t E, const float* __restrict__ jtab, int nJ, float* __restrict__ wig, int nW) {
    const int l = blockIdx.y;
    int off = 0, soff = nJ;
    for (int k = 0; k < l; ++k) {
        off += (2 * k + 1) * (2 * k + 1);
        soff += k + 1;
    }
    const float* __restrict__ J = jtab + off;
    const float* __restrict__ sg = jtab + soff;
    switch (l) {
        case 0: wigner_rows<0>(ang, E, J, sg, wig, nW, off); break;
        case 1: wigner_rows<1>(ang, E, J, sg, wig, nW, off); break;
        case 2: wigner_rows<2>(ang, E, J, sg, wig, nW, off); break;
        case 3: wigner_rows<3>(ang, E, J, sg, wig, nW, off); break;
        case 4: wigner_rows<4>(ang, E, J, sg, wig, nW, off); break;
        case 5: wigner_rows<5>(ang, E, J, sg, wig, nW, off); break;
        case 6: wigner_rows<6>(ang, E, J, sg, wig, nW, off); break;
        case 7: wigner_rows<7>(ang, E, J, sg, wig, nW, off); break;
        default: break;
    }
}

extern "C" int hg_edge_geometry(const float* pos, const int64_t* edge_index, const float* nbr_shift, int64_t E, float cutoff,
                                int num_radial, int lmax_wig, const float* jtab, float* rbf, float* wig, float* edge_len,
                                float* ang_scratch, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0) return 0;
    if (lmax_wig > 7) return hg_fail(-2, "hg_edge_geometry: lmax_wig > 7 not instantiated");
    hipStream_t st = (hipStream_t)stream;
    int nW = 0, nJ = 0;
    for (int l = 0; l <= lmax_wig; ++l) nW += (2 * l + 1) * (2 * l + 1);
    nJ = nW;
    float4* ang = reinterpret_cast<float4*>(ang_scratch);
    geometry_kernel<<<dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st>>>(pos, edge_index, nbr_shift, E, cutoff, num_radial, ang, rbf, edge_len);
    if (wig && E * (2 * lmax_wig + 1) <= 256 * 2048) {        // small crystal: every l in one launch
        wigner_all_kernel<<<dim3((unsigned)((E * (2 * lmax_wig + 1) + 255) / 256), (unsigned)(lmax_wig + 1)), 256, 0, st>>>(ang, E, jtab, nJ, wig, nW);
    } else if (wig) {
        int off = 0, soff = nJ;
        for (int l = 0; l <= lmax_wig; ++l) {
            const int N = 2 * l + 1;
            const unsigned grid = (unsigned)((E * N + 255) / 256);
            const float* J = jtab + off;
            const float* sg = jtab + soff;
            switch (l) {
                case 0: wigner_kernel<0><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 1: wigner_kernel<1><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 2: wigner_kernel<2><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 3: wigner_kernel<3><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 4: wigner_kernel<4><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 5: wigner_kernel<5><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 6: wigner_kernel<6><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
                case 7: wigner_kernel<7><<<grid, 256, 0, st>>>(ang, E, J, sg, wig, nW, off); break;
            }
            off += N * N;
            soff += l + 1;
        }
    }
    return hg_check_launch("hg_edge_geometry");
}

// ------------------------------------------------------------------------------------------------ other radial bases
// rbf_func = "gaussian" (hamgnn/models/hamgnn_conv.py:123-125 -> GaussianSmearing, utils/basis_functions.py:211-224, start 0, stop =
// cutoff, no inner cutoff) x the cosine cutoff of RadialBasisEdgeEncoding (nn/embeddings.py:93-97), from the edge lengths that
// hg_edge_geometry wrote.  fp64 internally, rounded once.  `offsets` = the reference's fp32 centres (torch.linspace is not n * delta
// to the last bit), `delta` = offsets[1] - offsets[0] in fp32 (the reference's width): both from the host, so both sides use the same numbers.
__global__ void gaussian_basis_kernel(const float* __restrict__ len, int64_t E, float cutoff, const float* __restrict__ offsets, float delta, int R,
                                      float* __restrict__ rbf) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * R) return;
    const int64_t e = idx / R;
    const int n = (int)(idx - e * R);
    const double r = (double)len[e];
    const double off = (double)offsets[n];
    const double fc = (r < (double)cutoff) ? 0.5 * (cos(M_PI * r / (double)cutoff) + 1.0) : 0.0;
    const double d = r - off;
    rbf[idx] = (float)(exp(-0.5 * d * d / ((double)delta * (double)delta)) * fc);
}

extern "C" int hg_radial_basis(const float* edge_len, int64_t E, int kind, float cutoff, const float* offsets, float delta, int num_radial, float* rbf,
                               void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0) return 0;
    if (kind != 1) return hg_fail(-2, "hg_radial_basis: kind 1 (gaussian) is built; bessel comes from hg_edge_geometry");
    if (num_radial < 2) return hg_fail(-2, "hg_radial_basis: num_radial >= 2");
    gaussian_basis_kernel<<<dim3((unsigned)((E * num_radial + 255) / 256)), 256, 0, (hipStream_t)stream>>>(edge_len, E, cutoff, offsets, delta, num_radial, rbf);
    return hg_check_launch("hg_radial_basis");
}

// ------------------------------------------------------------------------------------------------ gather + frame rotation
// out_s[e][i][a][u] = sum_b D_e^{l_i}[a][b] x_s[idx_s[e]][i][b][u].  Work item = (edge, source, group of 4 channels of one irrep):
// 2l+1 float4 loads (component stride mulp), (2l+1)^2 x 4 FMAs against the edge's Wigner block staged in LDS (broadcast
// reads, amortised over the 4 channels), 2l+1 float4 stores.  The group table is sorted by l and a wave covers 4 consecutive
// groups x 16 (edge, source) pairs, so a wavefront runs one -- at block seams two -- of the <L> paths.  (The r1 kernel used one
// channel per lane in layout order: a wavefront then spanned every l of the row and executed all seven paths serially -- it
// was VALU-issue bound at 1.3 TB/s instead of HBM bound.)
// grp_tab: int32[ngroups][4] = {l, planar offset of (component 0, first channel), mulp, valid channels (1..4)}.
template <int L>
__device__ __forceinline__ void rotate_group(const float* __restrict__ Dl, const float* __restrict__ xin, float* __restrict__ xout,
                                             int base, int mulp, int transpose, int nvalid) {
    constexpr int N = 2 * L + 1;
    f32x4 v[N];
#pragma unroll
    for (int b = 0; b < N; ++b) v[b] = *reinterpret_cast<const f32x4*>(xin + base + b * mulp);
    const f32x4 keep = (f32x4){1.f, nvalid > 1 ? 1.f : 0.f, nvalid > 2 ? 1.f : 0.f, nvalid > 3 ? 1.f : 0.f};
#pragma unroll
    for (int a = 0; a < N; ++a) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (!transpose) {
#pragma unroll
            for (int b = 0; b < N; ++b) acc += Dl[a * N + b] * v[b];
        } else {
#pragma unroll
            for (int b = 0; b < N; ++b) acc += Dl[b * N + a] * v[b];
        }
        *reinterpret_cast<f32x4*>(xout + base + a * mulp) = acc * keep;        // channel padding stays zero (zero-weight MFMA K-steps)
    }
}

#define RG_EB 16         // edges per workgroup: one frame staging + barrier per 16 x nsrc x ngroups work items
__global__ __launch_bounds__(256) void rotate_gather_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int64_t xs,
                                                            const int64_t* __restrict__ idx0, const int64_t* __restrict__ idx1,
                                                            const float* __restrict__ wig, int nW, const HgWigOff wo,
                                                            const int4* __restrict__ tab, int ngroups, int64_t E, int transpose,
                                                            float* __restrict__ out0, float* __restrict__ out1, int64_t os) {
    extern __shared__ float Dsm[];                             // [RG_EB][nW]
    const int64_t e0 = (int64_t)blockIdx.x * RG_EB;
    const int ne = (int)((E - e0) < RG_EB ? (E - e0) : RG_EB);
    for (int i = threadIdx.x; i < ne * nW; i += blockDim.x) Dsm[i] = wig[e0 * nW + i];
    __syncthreads();
    const int nsrc = x1 ? 2 : 1;
    const int npairs = RG_EB * nsrc;
    const int nsg = (ngroups + 3) >> 2;                        // super-groups of 4 consecutive groups
    for (int j = threadIdx.x; j < nsg * npairs * 4; j += blockDim.x) {
        const int sg = j / (npairs * 4);
        const int rem = j - sg * npairs * 4;
        const int pair = rem >> 2;
        const int gid = sg * 4 + (rem & 3);
        const int le = pair / nsrc;
        const int sidx = pair - le * nsrc;
        if (gid >= ngroups || le >= ne) continue;
        const int4 t = tab[gid];
        const int64_t e = e0 + le;
        const int64_t row = sidx ? (idx1 ? idx1[e] : e) : (idx0 ? idx0[e] : e);
        const float* __restrict__ xin = (sidx ? x1 : x0) + row * xs;
        float* __restrict__ xo = (sidx ? out1 : out0) + e * os;
        const float* __restrict__ Dl = Dsm + le * nW + wo.o[t.x];
        switch (t.x) {
            case 0: {
                const f32x4 keep = (f32x4){1.f, t.w > 1 ? 1.f : 0.f, t.w > 2 ? 1.f : 0.f, t.w > 3 ? 1.f : 0.f};
                *reinterpret_cast<f32x4*>(xo + t.y) = *reinterpret_cast<const f32x4*>(xin + t.y) * keep;
                break;
            }
            case 1: rotate_group<1>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 2: rotate_group<2>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 3: rotate_group<3>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 4: rotate_group<4>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 5: rotate_group<5>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 6: rotate_group<6>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;
            case 7: rotate_group<7>(Dl, xin, xo, t.y, t.z, transpose, t.w); break;      // su2 couplings of f-shell bases (gradient rows of the read-out)
            default: break;
        }
    }
}

extern "C" int hg_rotate_gather(const float* x0, const float* x1, int64_t x_stride, const int64_t* idx0, const int64_t* idx1,
                                const float* wig, int nW, const int32_t* wig_off, const int32_t* grp_tab, int ngroups, int64_t E,
                                int transpose, float* out0, float* out1, int64_t out_stride, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0) return 0;
    if ((x_stride & 3) || (out_stride & 3)) return hg_fail(-2, "hg_rotate_gather: row strides must be multiples of 4 floats (planar rows)");
    HgWigOff wo;
    for (int i = 0; i < 8; ++i) wo.o[i] = wig_off[i];
    const size_t lds = sizeof(float) * (size_t)nW * RG_EB;
    if (lds > 64 * 1024) return hg_fail(-2, "hg_rotate_gather: Wigner row too wide for the LDS staging");
    rotate_gather_kernel<<<dim3((unsigned)((E + RG_EB - 1) / RG_EB)), 256, lds, (hipStream_t)stream>>>(
        x0, x1, x_stride, idx0, idx1, wig, nW, wo, (const int4*)grp_tab, ngroups, E, transpose, out0, out1, out_stride);
    return hg_check_launch("hg_rotate_gather");
}
