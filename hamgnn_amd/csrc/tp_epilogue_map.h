// tp_epilogue_map.h -- which float4 of a segment's planar output block a lane of the edge kernel's epilogue serves (csrc/tp_stage.h:epilogue_is).
// Plain C++ without device-only constructs: the kernel includes it, and tests/test_epilogue_map.py compiles it into a host program that checks the map.
#pragma once

#if defined(__HIPCC__)
#define IS_EPI_FN __host__ __device__ __forceinline__
#else
#define IS_EPI_FN inline
#endif

// A segment's block holds NCO = 2 l + 1 components of `wend` channels (multiplicity + the padding slots of a last chunk): J = NCO * nq float4 units,
// nq = ceil(wend / 4) channel quads per component, unit j = a * nq + quad.  A wave step s serves the four units j = 4 s + g, one per lane group g
// (16 lanes = the tile's 16 edges), so every lane group works as long as units are left -- a unit of 16 channels per component and step left three of
// four groups idle in a 4-channel segment.  Each wave takes a contiguous range of steps: its stores are adjacent bytes of the row, and where the
// components follow each other without a gap (wend == out_mulp) a wave instruction writes 64 contiguous bytes per edge.
struct IsEpiMap {
    int nq, J;
    int s_begin, s_end;          // this wave's steps
    float inv_nq;
};

IS_EPI_FN IsEpiMap is_epi_map(int nco, int wend, int nwaves, int wave) {
    IsEpiMap m;
    m.nq = (wend + 3) >> 2;
    m.J = nco * m.nq;
    const int S = (m.J + 3) >> 2, per = (S + nwaves - 1) / nwaves;
    m.s_begin = wave * per;
    m.s_end = m.s_begin + per < S ? m.s_begin + per : S;
    m.inv_nq = 1.0f / (float)m.nq;
    return m;
}

// unit of (step s, lane group g) -> component a, first channel w; false: no unit left for this lane group (a, w are not to be used).
// j / nq through the reciprocal, as HG_DIV_P1 does for the staging's pieces: j < 2^9 and nq <= 16 (a tile holds at most 64 channels), so
// (j + 0.5) / nq is never within 0.03 of an integer and the float product rounds to the right side -- no integer division per unit and lane.
IS_EPI_FN bool is_epi_unit(const IsEpiMap& m, int s, int g, int& a, int& w) {
    const int j = 4 * s + g;
    a = (int)(((float)j + 0.5f) * m.inv_nq);
    w = 4 * (j - a * m.nq);
    return j < m.J;
}
