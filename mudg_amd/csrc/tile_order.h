// tile_order.h — which work item a workgroup takes: the XCD range split and the 8-row-group walk of the contraction kernels, once.
// Plain integer code that takes the block and grid numbers as arguments: the kernels (through common.h) and a host program
// (tests/test_tile_order_cpu.py) compile the same lines.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MUDG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MUDG_HD inline
#endif

// XCD-aware numbering of `total` work items: hardware places workgroup b on XCD b % 8; every XCD gets one contiguous range (the
// first total % 8 ranges one item longer), so that neighbouring items run on one XCD and share its L2.  Workgroup b of a grid that
// has one workgroup per item takes item first + b / 8; a persistent grid walks first + li, li = b / 8, b / 8 + stride, ... < count.
struct XcdRange { int first, count; };
MUDG_HD XcdRange xcd_range(int total, int xcd) {
    const int q8 = total >> 3, r8 = total & 7;
    return {xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8, q8 + (xcd < r8 ? 1 : 0)};
}

// Tile order inside a range: groups of 8 tile rows, column by column, so that the ~64 tiles an XCD runs at once form an 8 x 8
// patch (16 operand panels through its L2) instead of one 1 x 64 strip (65 panels) when N is wide.  The last group has ntm % 8 rows.
struct TileMN { int tm, tn; };
MUDG_HD TileMN group8_tile(int tile, int ntm, int ntn) {
    const int per = 8 * ntn, g = tile / per, first = g * 8;
    const int gsz = (ntm - first) < 8 ? (ntm - first) : 8;
    const int r = tile - g * per;
    const int tn = r / gsz;
    return {first + (r - tn * gsz), tn};
}
