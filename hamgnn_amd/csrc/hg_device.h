// hg_device.h -- device-side helpers shared by the kernels of libhamgnn_hip.so (gfx950): vector types, kernel-argument selects, LDS-DMA and
// fp32 MFMA wrappers, the index clamp and the Bloch phase of the k-space kernels, segment flags of the edge programs, the HG_PROF phase profiler.
// Included by every source that has a kernel.
#pragma once
#include "hg_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Kernel-argument arrays are only ever indexed through select chains: a dynamically indexed member makes the compiler copy the whole
// argument block into per-lane scratch -- 232 B x 2.1 M lanes = 0.5 GB of HBM writes per launch in the first build of the edge kernel.
template <class T>
__device__ __forceinline__ T hg_pick4(const T (&a)[4], int i) {
    return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3]));
}
template <class T>
__device__ __forceinline__ T hg_pick8(const T (&a)[8], int i) {
    return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : (i == 3 ? a[3] : (i == 4 ? a[4] : (i == 5 ? a[5] : (i == 6 ? a[6] : a[7]))))));
}

#ifndef HG_DMA_AUX
#define HG_DMA_AUX 2              // cache policy of the B-operand DMA: nt (streamed once per CU; keeps the shared A lines in L1; r1 A/B: -3 %)
#endif
// LDS-DMA: per-lane global address -> LDS at (wave-uniform base + lane * size); no VGPR round trip, counted by vmcnt
__device__ __forceinline__ void hg_dma16(const float* __restrict__ gsrc, float* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, HG_DMA_AUX);
}
__device__ __forceinline__ void hg_dma4(const float* __restrict__ gsrc, float* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

__device__ __forceinline__ f32x4 hg_mfma_f32_16x16x4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// v clamped into [0, n - 1]: what every entry of a caller's index table goes through before it indexes anything (spectra.hip)
__device__ __forceinline__ int hg_clampi(int v, int n) { return v < 0 ? 0 : v < n ? v : n - 1; }

// Bloch phase of an edge, (cos, sin) of 2 pi k . shift (kspace.hip, spectra.hip).  The angle and sincos in double, rounded to fp32 once: |k . shift|
// reaches tens of turns for long bonds, and sincosf loses the fraction.
__device__ __forceinline__ float2 hg_edge_phase(double kx, double ky, double kz, double sx, double sy, double sz) {
    const double ph = 6.283185307179586 * (kx * sx + ky * sy + kz * sz);
    double sd, cd;
    sincos(ph, &sd, &cd);
    return make_float2((float)cd, (float)sd);
}

// segment flags of the edge programs (tp_fused.hip, tp_is.hip; plan/program.py)
#define SEG_UNROTATE 1
#define SEG_ATOMIC 2             // (split launches only) the segment is one of TWO copies that share an output block: each adds its half of the items' sum
                                 // (plan.split_heavy_segments: the heaviest output irreps of a small crystal's launch on two workgroups; the rows are zero-filled by the host)
#define SEG_CENTRE 4             // (input-stationary schedule, un-rotated segments with l > 0) only the centre column (m = 0) of the tile is ever written: the
                                 // epilogue un-rotates that column alone, from row l of the Wigner block (plan/schedule_is.py)

// phase profiler of the edge kernels (HG_PROF builds only, tests/bench_tp.py --prof): per-wave shader-clock time between probes, summed over
// waves into the kernel's own __device__ array (hg_prof_read / hg_prof_is_read)
#ifdef HG_PROF
struct HgProf { unsigned long long t[12]; unsigned long long last; };
#define HG_PROF_ARG , HgProf& prof
#define HG_PROF_PASS , prof
#define HG_T(k)                                                      \
    do {                                                             \
        const unsigned long long t_ = __builtin_readcyclecounter();  \
        prof.t[k] += t_ - prof.last;                                 \
        prof.last = t_;                                              \
    } while (0)
#else
#define HG_PROF_ARG
#define HG_PROF_PASS
#define HG_T(k)
#endif
