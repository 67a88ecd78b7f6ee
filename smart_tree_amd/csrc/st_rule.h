// The wiring contract of the sparse convolutions: what both rulebook builders (rulebook.hip: hash tables, brick.hip:
// occupancy bricks) write and what sparse_conv.hip reads.  oracle/unet_oracle.py states the same rules in numpy.
#pragma once

#include "st_common.h"

// Kernel offset k = (kz*3 + ky)*3 + kx, components 0..2.  All tables are OUTPUT-stationary: nbr[k * stride + o] = input row
// that feeds output row o through offset k, or -1.
//   submanifold          in = out + (k - 1)
//   strided (k3 s2 p1)   in = 2*out - 1 + k
//   inverse              the strided pairs with the roles swapped, same k

// The strided rule.  A cloud whose largest fine coordinate along an axis is `ext` has coarse coordinates 0 .. ext >> 1
// (spconv's output size (ext + 1 - 1) / 2 + 1, exclusive); `level` halvings of a level-0 extent first.
__host__ __device__ inline int st_rule_omax(int ext, int level = 0) { return (ext >> level) >> 1; }

// Fine coordinate c pairs through offset component k with the coarse o for which 2*o - 1 + k = c: c + 1 - k must be even and
// o inside [0, omax].  *o is written in either case (callers build a look-up key from it before they know the answer).
__device__ __forceinline__ bool st_rule_axis(int c, int k, int omax, int* o) {
    const int n = c + 1 - k;
    *o = n >> 1;
    return !(n & 1) && n >= 0 && *o <= omax;
}
__device__ __forceinline__ bool st_rule_out(const int c[3], int kz, int ky, int kx, const int omax[3], int o[3]) {
    const bool z = st_rule_axis(c[0], kz, omax[0], &o[0]);
    const bool y = st_rule_axis(c[1], ky, omax[1], &o[1]);
    const bool x = st_rule_axis(c[2], kx, omax[2], &o[2]);
    return z && y && x;
}
__device__ __forceinline__ bool st_rule_out(const int c[3], int k, const int omax[3], int o[3]) {
    return st_rule_out(c, k / 9, (k / 3) % 3, k % 3, omax, o);
}

// Parity class and the tagged row order.  Which offsets of the pair set can have a partner depends only on the fine voxel's
// coordinate parity: per axis an even coordinate pairs through k = 1, an odd one through k = 0 and k = 2 -- 1, 2, 4 or 8 live
// offsets of 27.  The inverse convolution is launched over `order`: entry = fine row | (8 + class) << 28, rows grouped by
// class.  Top four bits 0 = nothing known about the row (a plain permutation is a valid order).
#define ST_RULE_ROW_LIMIT (1ll << 28)  // a tagged order holds rows below this
#define ST_RULE_ROW_MASK 0x0fffffff

__device__ __forceinline__ int st_rule_parity_class(int z, int y, int x) { return ((z & 1) << 2) | ((y & 1) << 1) | (x & 1); }
__device__ __forceinline__ int32_t st_rule_tag(int64_t row, int cls) { return (int32_t)((uint32_t)row | ((8u + (uint32_t)cls) << 28)); }
__device__ __forceinline__ int32_t st_rule_row(int32_t entry) { return entry & ST_RULE_ROW_MASK; }
// the 27-bit mask of offsets worth reading for the row of `entry` (all of them for an untagged row or another kernel size)
__device__ __forceinline__ uint32_t st_rule_live_offsets(int32_t entry, int K) {
    const uint32_t tag = (uint32_t)entry >> 28;
    if (!(tag & 8u) || K != 27) return 0xffffffffu;
    const uint32_t ax[3] = {(tag & 4u) ? 5u : 2u, (tag & 2u) ? 5u : 2u, (tag & 1u) ? 5u : 2u};  // z, y, x: {0,2} or {1}
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < 27; k++)
        if (((ax[0] >> (k / 9)) & (ax[1] >> ((k / 3) % 3)) & (ax[2] >> (k % 3))) & 1u) live |= 1u << k;
    return live;
}

// order[0 .. n) from the fine rows' coordinates (rulebook.hip).  pc [16]: the rows per class, counted by the builder's up/down
// kernel, then eight zeroed cursors.  n = min(*n_dev, cap) if n_dev is given, else cap; a non-zero *fail (optional): nothing is done.
void st_rule_parity_order(const int32_t* coords, int64_t cap, const int64_t* n_dev, const unsigned* fail, uint32_t* pc, int32_t* order,
                          hipStream_t stream);

// Which decoder rows a consumer of the INNER rows needs (block mode: every block carries a halo whose outputs are thrown away).
// Eval-mode BatchNorm is a per-channel affine, so an output row is a pure function of the rows its table names: a row nothing
// kept depends on can be left out without changing a bit of the rows that are kept.  The rule is conservative and reads no table:
//   box     per block (batch index) the bounding box [lo, hi] of its inner rows' level-0 coordinates; one level down the box is
//           [lo >> 1, (hi + 1) >> 1] (st_rule_need_box).  A block without an inner row has no box: none of its rows is needed.
//   margin  of a row at level l: its Chebyshev distance, in level-l voxels, from its block's level-l box (0 inside).
//   subm    in = out + (k - 1): an output at margin m reads inputs at margin <= m + 1.
//   inverse a fine c pairs with coarse o where 2 o - 1 + k = c, so o is floor(c / 2) or ceil(c / 2).  With lo - m <= c <= hi + m:
//           o >= floor((lo - m) / 2) >= (lo >> 1) - ceil(m / 2) and o <= ceil((hi + m) / 2) <= ((hi + 1) >> 1) + ceil(m / 2) --
//           coarse margin <= ceil(m / 2) against the halved box.
//   clip    the clip at the cloud's extent (st_rule_omax) only removes pairs.
// Walking a level's decoder backwards from the rows its consumer keeps (margin <= a[l], a[0] = 0: the inner rows themselves):
//   Tail.sequence.3, Tail.identity.0     rows with margin <= a[l]
//   Tail.sequence.0                      <= a[l] + 1   (sequence.3 is submanifold)
//   Decode.sequence.0 (level-l outputs)  <= a[l] + 2   (sequence.0 is submanifold and reads cat(skip, decoded))
//   Tail.sequence.3 one level down       <= a[l + 1] = ceil((a[l] + 2) / 2)   (Decode is the inverse convolution)
// -> a = 0, 1, 2, 2, 2, ...  The encoder side (Head, Encode) has a receptive field wider than any halo and runs in full.
#define ST_RULE_NEED_CLASSES 3  // margin <= a[l], = a[l] + 1, = a[l] + 2: the three launch prefixes of a level's need list
__host__ __device__ inline int st_rule_need_base(int level) {
    int a = 0;
    for (int l = 0; l < level; l++) a = (a + 2 + 1) >> 1;
    return a;
}
// the level-`level` box of a level-0 box side [lo, hi]
__host__ __device__ inline void st_rule_need_box(int lo, int hi, int level, int* blo, int* bhi) {
    *blo = lo >> level;                       // `level` floor-halvings
    *bhi = (hi + (1 << level) - 1) >> level;  // `level` times (hi + 1) >> 1
}
// margin class of a row at level `level`: 0 .. ST_RULE_NEED_CLASSES - 1, or ST_RULE_NEED_CLASSES = no convolution of the decoder needs it.
// lo / hi: the block's level-0 box (lo > hi: the block has none).
__host__ __device__ inline int st_rule_need_class(const int c[3], const int lo[3], const int hi[3], int level) {
    int m = 0;
    for (int a = 0; a < 3; a++) {
        if (lo[a] > hi[a]) return ST_RULE_NEED_CLASSES;
        int blo, bhi;
        st_rule_need_box(lo[a], hi[a], level, &blo, &bhi);
        const int d = c[a] < blo ? blo - c[a] : (c[a] > bhi ? c[a] - bhi : 0);
        m = d > m ? d : m;
    }
    const int over = m - st_rule_need_base(level);
    return over <= 0 ? 0 : (over < ST_RULE_NEED_CLASSES ? over : ST_RULE_NEED_CLASSES);
}

// Per-cloud extent.  A cloud's coarse sets are clipped at its OWN extent, so they do not depend on what else is in the batch:
// ext[seg * 3 + axis] = largest coordinate.  A workgroup reduces into m (LDS, nseg * 3 words), then one atomicMax per word.
__device__ __forceinline__ void st_ext_clear(int* m, int nseg) {
    for (int i = threadIdx.x; i < nseg * 3; i += blockDim.x) m[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void st_ext_offer(int* m, int seg, int z, int y, int x) {
    if (z > m[3 * seg]) atomicMax(&m[3 * seg], z);
    if (y > m[3 * seg + 1]) atomicMax(&m[3 * seg + 1], y);
    if (x > m[3 * seg + 2]) atomicMax(&m[3 * seg + 2], x);
}
__device__ __forceinline__ void st_ext_flush(const int* m, int nseg, int* ext) {
    __syncthreads();
    for (int i = threadIdx.x; i < nseg * 3; i += blockDim.x) if (m[i]) atomicMax(&ext[i], m[i]);
}
