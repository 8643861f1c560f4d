"""The tile order of the contraction kernels (mudg_amd/csrc/tile_order.h: xcd_range, group8_tile), run on the host.

The header is plain integer code that takes the block and grid numbers as arguments, so the very lines the kernels compile are
compiled here into a small program with its own main and run: no GPU, no HIP call.  Built twice, plainly and with the address and
undefined-behaviour sanitizers on the host side.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "tile_order.h"
#include <cstdio>
#include <vector>

// one workgroup per tile (gemm.hip, wgemm_kernel, hgeglu_kernel, wq_kernel): block b takes tile first + b / 8 of its XCD's range
static int one_tile(int ntm, int ntn) {
    const int grid = ntm * ntn;
    std::vector<int> seen(grid, 0);
    for (int b = 0; b < grid; ++b) {
        const XcdRange r = xcd_range(grid, b & 7);
        if ((b >> 3) >= r.count) { std::printf("one-tile %d x %d: block %d beyond its range\n", ntm, ntn, b); return 1; }
        const TileMN t = group8_tile(r.first + (b >> 3), ntm, ntn);
        if (t.tm < 0 || t.tm >= ntm || t.tn < 0 || t.tn >= ntn) { std::printf("one-tile %d x %d: block %d -> (%d, %d)\n", ntm, ntn, b, t.tm, t.tn); return 1; }
        seen[t.tm * ntn + t.tn] += 1;
    }
    for (int i = 0; i < grid; ++i)
        if (seen[i] != 1) { std::printf("one-tile %d x %d: tile (%d, %d) visited %d times\n", ntm, ntn, i / ntn, i % ntn, seen[i]); return 1; }
    return 0;
}

// persistent (pgemm.hip, wgemm_pkernel): the workgroups of XCD x walk first + li, li = b / 8, + stride, ... < count, where stride is the
// number of workgroups the hardware places on that XCD
static int persistent(int ntm, int ntn, int grid) {
    const int tiles = ntm * ntn;
    std::vector<int> seen(tiles, 0);
    for (int b = 0; b < grid; ++b) {
        const int xcd = b & 7, stride = (grid - xcd + 7) >> 3;
        const XcdRange r = xcd_range(tiles, xcd);
        for (int li = b >> 3; li < r.count; li += stride) {
            const TileMN t = group8_tile(r.first + li, ntm, ntn);
            if (t.tm < 0 || t.tm >= ntm || t.tn < 0 || t.tn >= ntn) { std::printf("persistent %d x %d, grid %d: (%d, %d)\n", ntm, ntn, grid, t.tm, t.tn); return 1; }
            seen[t.tm * ntn + t.tn] += 1;
        }
    }
    for (int i = 0; i < tiles; ++i)
        if (seen[i] != 1) { std::printf("persistent %d x %d, grid %d: tile (%d, %d) visited %d times\n", ntm, ntn, grid, i / ntn, i % ntn, seen[i]); return 1; }
    return 0;
}

int main() {
    const int shapes[][2] = {{1, 1}, {7, 3}, {8, 2}, {9, 5}, {17, 1}, {300, 2}};
    const int grids[] = {8, 13, 256};
    int bad = 0, runs = 0;
    for (const auto& s : shapes) {
        bad += one_tile(s[0], s[1]); ++runs;
        for (const int g : grids)
            if (g <= s[0] * s[1]) { bad += persistent(s[0], s[1], g); ++runs; }
    }
    std::printf("%d walks, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_every_tile_is_visited_exactly_once(tmp_path, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed: the program is compiled as the kernels are"
    src = tmp_path / "tile_order_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "tile_order_main"
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "mudg_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("17 walks, 0 bad"), run.stdout          # 6 one-tile walks + 11 persistent ones (grid <= tiles)
