// neighbour.hip -- the periodic neighbour list of HamGNN_pre.build_internal_graph on the device (gfx950): the kernels behind hamgnn_amd/internal_graph.py.
// Replaces the reference's host-side (ASE) graph construction, BaseModel.generate_graph.
#include "hg_device.h"

// ------------------------------------------------------------------------------------------------ periodic neighbour list (HamGNN_pre.build_internal_graph)
// BaseModel.generate_graph (hamgnn/models/base_model.py:237-288) on the device: all directed periodic pairs (i, j, S) of one crystal with
// |pos_j + S cell - pos_i| < r_i + r_j (fp64 from the fp32 inputs, strict), (i, i, 0) excluded.  A cell list in FRACTIONAL coordinates: along lattice
// direction d the cell is cut into nb_d = floor(height_d / rcut) bins (rcut = the largest r_i + r_j of the batch, a hair widened), so a neighbour lies in
// the same or an adjacent bin and the three bins are visited with wrap-around (the wrap is the image shift); a direction with fewer than three bins is ONE
// bin whose ceil(rcut / height_d) images on either side are looped over.  Atoms are wrapped into the home cell first (wrap = floor of the fractional
// coordinate), the emitted shift S = image - wrap_j + wrap_i refers to the positions as given.  Every edge is ONE int64 key
//     i << 39 | j << 15 | (S0 + 16) << 10 | (S1 + 16) << 5 | (S2 + 16)            (atoms < 2^24, |S| <= 15)
// whose ascending order is the canonical edge order (i, j, S0, S1, S2); a centre's keys go into its own segment (count pass, prefix sum by the caller,
// fill pass), one thread per centre in a fixed loop order -- nothing depends on scheduling.  Integer atomics only raise error flags.
#define NL_IDX_BITS 24
#define NL_S_OFF 16
#define NL_S_MAX 15
#define NL_MAX_BINS_DIR 1024
enum { NL_BAD_CELL = 1, NL_BAD_RANGE = 2, NL_OVERFLOW = 4, NL_BAD_INPUT = 8 };
// cpar [B][20] doubles: cell rows a0 a1 a2 (9) | inv (9): fractional coordinate d of p = sum_k p[k] inv[3 k + d] | rcut | -
// ipar [B][8] int32:   nb0 nb1 nb2 | nimg0 nimg1 nimg2 | first bin of the crystal | bins of the crystal

__global__ void nl_setup_kernel(const float* __restrict__ cell, const int64_t* __restrict__ atom_ptr, const double* __restrict__ rcut_p, int B,
                                double* __restrict__ cpar, int32_t* __restrict__ ipar, int32_t* __restrict__ flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double a[9], c[9];
    for (int k = 0; k < 9; ++k) a[k] = (double)cell[9 * b + k];
    for (int d = 0; d < 3; ++d) {                               // c_d = a_{d+1} x a_{d+2}
        const double* u = a + 3 * ((d + 1) % 3);
        const double* v = a + 3 * ((d + 2) % 3);
        c[3 * d + 0] = u[1] * v[2] - u[2] * v[1];
        c[3 * d + 1] = u[2] * v[0] - u[0] * v[2];
        c[3 * d + 2] = u[0] * v[1] - u[1] * v[0];
    }
    const double det = a[0] * c[0] + a[1] * c[1] + a[2] * c[2];
    const double rcut = rcut_p[0] * (1.0 + 1e-9);
    int bad = 0;
    if (!(fabs(det) > 0.0) || !isfinite(det) || !(rcut > 0.0) || !isfinite(rcut)) bad |= NL_BAD_CELL;
    int nb[3] = {1, 1, 1}, nimg[3] = {0, 0, 0};
    if (!bad) {
        for (int d = 0; d < 3; ++d) {
            const double h = fabs(det) / sqrt(c[3 * d] * c[3 * d] + c[3 * d + 1] * c[3 * d + 1] + c[3 * d + 2] * c[3 * d + 2]);
            const double q = h / rcut;
            if (q >= 3.0) {
                nb[d] = (int)fmin(q, (double)NL_MAX_BINS_DIR);
            } else {
                const double m = ceil(rcut / h);
                if (!(m <= (double)NL_S_MAX)) bad |= NL_BAD_RANGE;
                else nimg[d] = (int)m;
            }
        }
        // no more bins than atoms (or 27): the caller sizes the bin table as N + 27 B without reading anything back; wider bins stay valid
        const int64_t n_b = atom_ptr[b + 1] - atom_ptr[b];
        for (int it = 0; it < 3 * NL_MAX_BINS_DIR; ++it) {
            if ((int64_t)nb[0] * nb[1] * nb[2] <= n_b) break;
            const int d = nb[0] >= nb[1] ? (nb[0] >= nb[2] ? 0 : 2) : (nb[1] >= nb[2] ? 1 : 2);
            if (nb[d] <= 3) break;
            --nb[d];
        }
    }
    if (bad) {
        nb[0] = nb[1] = nb[2] = 1;
        nimg[0] = nimg[1] = nimg[2] = 0;
        atomicOr(flags, bad);
    }
    double* cp = cpar + 20 * (int64_t)b;
    for (int k = 0; k < 9; ++k) cp[k] = a[k];
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) cp[9 + 3 * k + d] = bad ? 0.0 : c[3 * d + k] / det;
    cp[18] = rcut;
    cp[19] = 0.0;
    int32_t* ip = ipar + 8 * (int64_t)b;
    for (int d = 0; d < 3; ++d) { ip[d] = nb[d]; ip[3 + d] = nimg[d]; }
    ip[6] = 0;
    ip[7] = nb[0] * nb[1] * nb[2];
}

// first bin of every crystal: a serial prefix over B small integers (B = crystals of the batch)
__global__ void nl_bin_offsets_kernel(int32_t* __restrict__ ipar, int B, int64_t bins_cap, int32_t* __restrict__ flags) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t off = 0;
    for (int b = 0; b < B; ++b) {
        int32_t* ip = ipar + 8 * (int64_t)b;
        if (off + ip[7] > bins_cap) {                          // cannot happen with bins_cap >= N + 27 B; one bin then, never an index past the table
            ip[0] = ip[1] = ip[2] = 1;
            ip[7] = 1;
            atomicOr(flags, NL_OVERFLOW);
            if (off + 1 > bins_cap) off = bins_cap - 1;
        }
        ip[6] = (int32_t)off;
        off += ip[7];
    }
}

__global__ void nl_bin_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch, int64_t N, int B, const double* __restrict__ cpar,
                              const int32_t* __restrict__ ipar, int64_t* __restrict__ bin_id, int32_t* __restrict__ wrap, int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int64_t b = batch ? batch[i] : 0;
    int bad = 0;
    if (b < 0 || b >= B) { bad = NL_BAD_INPUT; b = 0; }
    const double* cp = cpar + 20 * b;
    const int32_t* ip = ipar + 8 * b;
    const double p[3] = {(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]};
    int64_t bin = 0;
    for (int d = 0; d < 3; ++d) {
        double f = p[0] * cp[9 + d] + p[1] * cp[12 + d] + p[2] * cp[15 + d];
        if (!(fabs(f) < 1.0e9)) { bad = NL_BAD_INPUT; f = 0.0; }          // NaN / inf / an atom a billion cells away
        const double w = floor(f);
        const int nb = ip[d];
        int k = (int)((f - w) * (double)nb);
        k = k < 0 ? 0 : (k >= nb ? nb - 1 : k);
        bin = bin * nb + k;
        wrap[3 * i + d] = (int32_t)w;
    }
    bin_id[i] = (int64_t)ip[6] + bin;
    if (bad) atomicOr(flags, bad);
}

// one thread per centre; keys == NULL: count pass (counts[i]); else fill pass into keys[seg_ptr[i] ..), never past `capacity` nor past the centre's own segment
__global__ void nl_pairs_kernel(const float* __restrict__ pos, const double* __restrict__ radius, const int64_t* __restrict__ batch,
                                const double* __restrict__ cpar, const int32_t* __restrict__ ipar, const int64_t* __restrict__ bin_id,
                                const int32_t* __restrict__ wrap, const int64_t* __restrict__ bin_start, const int64_t* __restrict__ bin_atoms, int64_t N,
                                int B, int64_t bins_cap, const int64_t* __restrict__ seg_ptr, int64_t capacity, int64_t* __restrict__ counts,
                                int64_t* __restrict__ keys, int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int64_t b = batch ? batch[i] : 0;
    if (b < 0 || b >= B) b = 0;                                 // (flagged by the binning pass)
    const double* cp = cpar + 20 * b;
    const int32_t* ip = ipar + 8 * b;
    const int nb0 = ip[0], nb1 = ip[1], nb2 = ip[2];
    const int64_t boff = ip[6];
    int64_t lb = bin_id[i] - boff;
    const int b2 = (int)(lb % nb2); lb /= nb2;
    const int b1 = (int)(lb % nb1);
    const int b0 = (int)(lb / nb1);
    const int r0 = nb0 >= 3 ? 1 : ip[3], r1 = nb1 >= 3 ? 1 : ip[4], r2 = nb2 >= 3 ? 1 : ip[5];
    const double pi0 = (double)pos[3 * i], pi1 = (double)pos[3 * i + 1], pi2 = (double)pos[3 * i + 2];
    const double ri = radius[i];
    const int wi0 = wrap[3 * i], wi1 = wrap[3 * i + 1], wi2 = wrap[3 * i + 2];
    int64_t out = 0, seg0 = 0, seg1 = 0;
    if (keys) {
        seg0 = seg_ptr[i];
        seg1 = seg_ptr[i + 1];
        if (seg1 > capacity) seg1 = capacity;
    }
    int bad = 0;
    for (int o0 = -r0; o0 <= r0; ++o0) {
        int c0 = 0, m0 = o0;
        if (nb0 >= 3) { c0 = b0 + o0; m0 = 0; if (c0 < 0) { c0 += nb0; m0 = -1; } else if (c0 >= nb0) { c0 -= nb0; m0 = 1; } }
        for (int o1 = -r1; o1 <= r1; ++o1) {
            int c1 = 0, m1 = o1;
            if (nb1 >= 3) { c1 = b1 + o1; m1 = 0; if (c1 < 0) { c1 += nb1; m1 = -1; } else if (c1 >= nb1) { c1 -= nb1; m1 = 1; } }
            for (int o2 = -r2; o2 <= r2; ++o2) {
                int c2 = 0, m2 = o2;
                if (nb2 >= 3) { c2 = b2 + o2; m2 = 0; if (c2 < 0) { c2 += nb2; m2 = -1; } else if (c2 >= nb2) { c2 -= nb2; m2 = 1; } }
                const int64_t g = boff + ((int64_t)c0 * nb1 + c1) * nb2 + c2;
                if (g < 0 || g >= bins_cap) { bad |= NL_OVERFLOW; continue; }
                int64_t t0 = bin_start[g], t1 = bin_start[g + 1];
                if (t0 < 0) t0 = 0;
                if (t1 > N) t1 = N;
                for (int64_t t = t0; t < t1; ++t) {
                    const int64_t j = bin_atoms[t];
                    if (j < 0 || j >= N) { bad |= NL_BAD_INPUT; continue; }
                    const int s0 = m0 - wrap[3 * j] + wi0, s1 = m1 - wrap[3 * j + 1] + wi1, s2 = m2 - wrap[3 * j + 2] + wi2;
                    if (j == i && s0 == 0 && s1 == 0 && s2 == 0) continue;
                    const double vx = (double)pos[3 * j] + ((double)s0 * cp[0] + (double)s1 * cp[3] + (double)s2 * cp[6]) - pi0;
                    const double vy = (double)pos[3 * j + 1] + ((double)s0 * cp[1] + (double)s1 * cp[4] + (double)s2 * cp[7]) - pi1;
                    const double vz = (double)pos[3 * j + 2] + ((double)s0 * cp[2] + (double)s1 * cp[5] + (double)s2 * cp[8]) - pi2;
                    if (!(sqrt(vx * vx + vy * vy + vz * vz) < ri + radius[j])) continue;
                    if (s0 < -NL_S_MAX || s0 > NL_S_MAX || s1 < -NL_S_MAX || s1 > NL_S_MAX || s2 < -NL_S_MAX || s2 > NL_S_MAX) { bad |= NL_BAD_RANGE; continue; }
                    if (keys) {
                        if (seg0 + out < seg1)
                            keys[seg0 + out] = (i << 39) | (j << 15) | ((int64_t)(s0 + NL_S_OFF) << 10) | ((int64_t)(s1 + NL_S_OFF) << 5) | (int64_t)(s2 + NL_S_OFF);
                        else
                            bad |= NL_OVERFLOW;
                    }
                    ++out;
                }
            }
        }
    }
    if (!keys) counts[i] = out;
    else if (out != seg_ptr[i + 1] - seg0) bad |= NL_OVERFLOW;  // the two passes disagree (the inputs changed in between), or the segment was cut at `capacity`
    if (bad) atomicOr(flags, bad);
}

__global__ void nl_decode_kernel(const int64_t* __restrict__ keys, int64_t E, const float* __restrict__ cell, const int64_t* __restrict__ batch, int64_t N,
                                 int B, int64_t* __restrict__ edge_index, int64_t* __restrict__ cell_shift, float* __restrict__ nbr_shift) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t k = keys[e];
    int64_t i = (k >> 39) & ((1 << NL_IDX_BITS) - 1), j = (k >> 15) & ((1 << NL_IDX_BITS) - 1);
    const int s[3] = {(int)((k >> 10) & 31) - NL_S_OFF, (int)((k >> 5) & 31) - NL_S_OFF, (int)(k & 31) - NL_S_OFF};
    if (i >= N) i = N - 1;                                      // (keys come from the fill pass: in range; a foreign key must not index past the tables)
    if (j >= N) j = N - 1;
    int64_t b = batch ? batch[i] : 0;
    if (b < 0 || b >= B) b = 0;
    edge_index[e] = i;
    edge_index[E + e] = j;
    const float* c = cell + 9 * b;
    for (int d = 0; d < 3; ++d) {
        cell_shift[3 * e + d] = s[d];
        nbr_shift[3 * e + d] = (float)((double)s[0] * (double)c[d] + (double)s[1] * (double)c[3 + d] + (double)s[2] * (double)c[6 + d]);
    }
}

extern "C" int hg_neighbour_bin(const float* pos, const float* cell, const int64_t* batch, const int64_t* atom_ptr, const double* rcut, int64_t N, int B,
                                int64_t bins_cap, double* cpar, int32_t* ipar, int64_t* bin_id, int32_t* wrap, int32_t* flags, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (N <= 0 || B <= 0) return 0;
    if (N > ((int64_t)1 << NL_IDX_BITS)) return hg_fail(-2, "hg_neighbour_bin: at most 2^24 atoms per batch (the packed edge key holds 24 bits per atom index)");
    if (bins_cap < N + 27 * (int64_t)B) return hg_fail(-2, "hg_neighbour_bin: bins_cap must be at least N + 27 B");
    hipStream_t st = (hipStream_t)stream;
    nl_setup_kernel<<<dim3((unsigned)((B + 63) / 64)), 64, 0, st>>>(cell, atom_ptr, rcut, B, cpar, ipar, flags);
    nl_bin_offsets_kernel<<<1, 64, 0, st>>>(ipar, B, bins_cap, flags);
    nl_bin_kernel<<<dim3((unsigned)((N + 255) / 256)), 256, 0, st>>>(pos, batch, N, B, cpar, ipar, bin_id, wrap, flags);
    return hg_check_launch("hg_neighbour_bin");
}

extern "C" int hg_neighbour_pairs(const float* pos, const double* radius, const int64_t* batch, const double* cpar, const int32_t* ipar, const int64_t* bin_id,
                                  const int32_t* wrap, const int64_t* bin_start, const int64_t* bin_atoms, int64_t N, int B, int64_t bins_cap,
                                  const int64_t* seg_ptr, int64_t capacity, int64_t* counts, int64_t* keys, int32_t* flags, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (N <= 0 || B <= 0) return 0;
    if (N > ((int64_t)1 << NL_IDX_BITS)) return hg_fail(-2, "hg_neighbour_pairs: at most 2^24 atoms per batch");
    if (keys ? (!seg_ptr || capacity < 0) : !counts) return hg_fail(-2, "hg_neighbour_pairs: the count pass needs `counts`, the fill pass `seg_ptr` and a capacity");
    nl_pairs_kernel<<<dim3((unsigned)((N + 63) / 64)), 64, 0, (hipStream_t)stream>>>(pos, radius, batch, cpar, ipar, bin_id, wrap, bin_start, bin_atoms, N, B, bins_cap,
                                                                                       seg_ptr, capacity, counts, keys, flags);
    return hg_check_launch("hg_neighbour_pairs");
}

extern "C" int hg_neighbour_decode(const int64_t* keys, int64_t E, const float* cell, const int64_t* batch, int64_t N, int B, int64_t* edge_index,
                                   int64_t* cell_shift, float* nbr_shift, void* stream) {
    HgDeviceGuard dev_guard(stream);
    if (E <= 0) return 0;
    if (N <= 0 || B <= 0) return hg_fail(-2, "hg_neighbour_decode: edges without atoms");
    nl_decode_kernel<<<dim3((unsigned)((E + 255) / 256)), 256, 0, (hipStream_t)stream>>>(keys, E, cell, batch, N, B, edge_index, cell_shift, nbr_shift);
    return hg_check_launch("hg_neighbour_decode");
}
