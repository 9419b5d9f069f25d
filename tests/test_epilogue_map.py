"""The lane map of the edge kernel's epilogue (hamgnn_amd/csrc/tp_epilogue_map.h: wave step s, lane group g -> component a, first channel w) checked on the host:
the header holds no device-only construct, so a stand-alone C++ program includes the very file the kernel includes.  For l = 0 .. 6, wend = 4, 8, .. 64 (and the
ragged widths in between, which a chunk that is not the last can have) and workgroups of 4 and 8 waves:
  * every (component, channel quad) of the segment's planar block is produced exactly once over all waves and steps, none outside the block;
  * the units of a wave are consecutive float4s of the block, and the waves' ranges follow each other in wave order;
  * the reciprocal that replaces j / nq gives the quotient for every j < 2^9 and nq <= 16, also with the reciprocal off by a few ulps either way."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "tp_epilogue_map.h"

int main() {
    long cases = 0, units = 0;
    for (int l = 0; l <= 6; ++l)
        for (int wend = 1; wend <= 64; ++wend)
            for (int nw = 4; nw <= 8; nw += 4) {
                const int nco = 2 * l + 1, nq = (wend + 3) / 4, J = nco * nq;
                std::vector<int> seen(J, 0);
                int next = 0;                                  // the float4 the next wave has to start at
                for (int wave = 0; wave < nw; ++wave) {
                    const IsEpiMap m = is_epi_map(nco, wend, nw, wave);
                    if (m.nq != nq || m.J != J) { std::printf("FAIL sizes l %d wend %d\n", l, wend); return 1; }
                    for (int s = m.s_begin; s < m.s_end; ++s)
                        for (int g = 0; g < 4; ++g) {
                            int a = -1, w = -1;
                            if (!is_epi_unit(m, s, g, a, w)) {
                                if (4 * s + g < J) { std::printf("FAIL idle lane inside the block l %d wend %d nw %d\n", l, wend, nw); return 1; }
                                continue;
                            }
                            if (a < 0 || a >= nco || w < 0 || (w & 3) || w >= wend) { std::printf("FAIL outside l %d wend %d nw %d: a %d w %d\n", l, wend, nw, a, w); return 1; }
                            const int j = a * nq + w / 4;
                            if (j != next) { std::printf("FAIL not consecutive l %d wend %d nw %d wave %d: unit %d, expected %d\n", l, wend, nw, wave, j, next); return 1; }
                            ++next, ++seen[j], ++units;
                        }
                }
                for (int j = 0; j < J; ++j)
                    if (seen[j] != 1) { std::printf("FAIL l %d wend %d nw %d: unit %d produced %d times\n", l, wend, nw, j, seen[j]); return 1; }
                ++cases;
            }
    // the reciprocal itself, beyond the sizes above: every j < 2^9, nq <= 16, the reciprocal up to 4 ulps off
    for (int nq = 1; nq <= 16; ++nq) {
        IsEpiMap m = is_epi_map(1, 4 * nq, 4, 0);
        for (int d = -4; d <= 4; ++d) {
            float inv = 1.0f / (float)nq;
            for (int k = 0; k < (d < 0 ? -d : d); ++k) inv = std::nextafterf(inv, d < 0 ? 0.f : 2.f);
            m.inv_nq = inv;
            m.J = 1 << 9;
            for (int j = 0; j < (1 << 9); ++j) {
                int a, w;
                is_epi_unit(m, j >> 2, j & 3, a, w);
                if (a != j / nq || w != 4 * (j % nq)) { std::printf("FAIL reciprocal nq %d j %d ulps %d: a %d w %d\n", nq, j, d, a, w); return 1; }
            }
        }
    }
    std::printf("OK cases %ld units %ld\n", cases, units);
    return 0;
}
"""


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    return None


def test_epilogue_lane_map_covers_every_float4_once(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    src = tmp_path / "main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "epilogue_map")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hamgnn_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("OK cases 896 "), r.stdout + r.stderr      # 7 l x 64 widths x 2 workgroup sizes
    # sum over l, wend of (2 l + 1) ceil(wend / 4), for both workgroup sizes
    want = 2 * sum((2 * l + 1) * ((w + 3) // 4) for l in range(7) for w in range(1, 65))
    assert int(r.stdout.split()[4]) == want
