// Half-precision sparse convolution for mixed-precision (autocast float16) training:
//
//   st_sparse_conv_h_fwd     y[o] = sum_k cat(x0, x1)[nbr[k][o]] . W[k]     x0, x1, W [K][cin][cout], y: IEEE half
//   st_sparse_conv_wgrad_h   dW[k] = sum over live pairs (i = nbr[k][o], o) of cat(x0, x1)[i]^T dy[o]    x, dy half, dW float32
//   st_move_rows_h           rows of 2-byte elements moved by a permutation (the spatial order into / out of the network)
//
// The data gradient is st_sparse_conv_h_fwd over the transposed table with transposed weights (model/sparse_grad.py).
// Replaces what spconv's SubMConv3d / SparseConv3d / SparseInverseConv3d run forward and backward when the reference trains under
// torch.cuda.amp.autocast (smart_tree/model/train.py:24-58, conf/training.yaml fp16: True).
//
// Arithmetic: products of two halves are exact in float32; every sum is float32 (fmaf chains on the vector form,
// v_mfma_f32_16x16x32_f16 on the matrix form); the forward rounds once to half at the store, the weight gradient stays float32.
// Nothing clamps: an inf / NaN operand reaches every sum it takes part in (loss scaling needs an overflowed dy to show up in dx / dW).
// Weights are read in the plain [K][cin][cout] layout, as autograd holds them (no per-step permutation).
#include "st_common.h"

typedef _Float16 sth_h;
typedef _Float16 sth_v8h __attribute__((ext_vector_type(8)));
typedef _Float16 sth_v4h __attribute__((ext_vector_type(4)));
typedef float sth_v4f __attribute__((ext_vector_type(4)));

#define HC_BLOCK 256

// Which form a (cin, cout) takes.  16-wide column tiles and 32-deep channel chunks waste at most half of the matrix core's work at
// 16 channels; below that (3 -> 8 input conv, 8-channel level 0, the 8 -> 4 -> {1, 3, 2} heads) the vector form does less work.
static inline bool hconv_matrix_form(int cin, int cout) { return cin >= 16 && cout >= 16; }

// ------------------------------------------------------------------------------- forward, vector form ---
// One lane per output row and COT output channels; offsets ascending, input channels ascending, one fmaf per product.  Weight
// addresses are wave-uniform (scalar loads).  V4: a row is read in 8-byte pieces of 4 channels (cin and c0 multiples of 4, aligned).
template <int COT, bool V4>
__global__ void __launch_bounds__(HC_BLOCK) k_hconv_vec(const sth_h* __restrict__ x0, int c0, const sth_h* __restrict__ x1, int cin,
                                                        const int32_t* __restrict__ nbr, int K, int64_t n_out, int64_t nstride,
                                                        const sth_h* __restrict__ w, int cout, int co_tiles, sth_h* __restrict__ y) {
    const int co0 = (int)(blockIdx.x % (unsigned)co_tiles) * COT;
    const int64_t o = (int64_t)(blockIdx.x / (unsigned)co_tiles) * HC_BLOCK + threadIdx.x;
    if (o >= n_out) return;
    const int nco = cout - co0 < COT ? cout - co0 : COT;
    const int c1 = cin - c0;
    float acc[COT];
#pragma unroll
    for (int c = 0; c < COT; c++) acc[c] = 0.0f;
    for (int k = 0; k < K; k++) {
        const int idx = nbr ? nbr[(int64_t)k * nstride + o] : (int)o;
        if (idx < 0) continue;
        const sth_h* __restrict__ wk = w + (int64_t)k * cin * cout + co0;
        if (V4) {
            for (int ci = 0; ci < cin; ci += 4) {
                const sth_h* row = ci < c0 ? x0 + (int64_t)idx * c0 + ci : x1 + (int64_t)idx * c1 + (ci - c0);
                const sth_v4h v = *reinterpret_cast<const sth_v4h*>(row);
                const float xs[4] = {(float)v.x, (float)v.y, (float)v.z, (float)v.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const sth_h* wr = wk + (int64_t)(ci + j) * cout;
                    if (nco == COT) {
#pragma unroll
                        for (int c = 0; c < COT; c++) acc[c] = fmaf(xs[j], (float)wr[c], acc[c]);
                    } else {
                        for (int c = 0; c < nco; c++) acc[c] = fmaf(xs[j], (float)wr[c], acc[c]);
                    }
                }
            }
        } else {
            for (int ci = 0; ci < cin; ci++) {
                const float xv = (float)(ci < c0 ? x0[(int64_t)idx * c0 + ci] : x1[(int64_t)idx * c1 + (ci - c0)]);
                const sth_h* wr = wk + (int64_t)ci * cout;
                if (nco == COT) {
#pragma unroll
                    for (int c = 0; c < COT; c++) acc[c] = fmaf(xv, (float)wr[c], acc[c]);
                } else {
                    for (int c = 0; c < nco; c++) acc[c] = fmaf(xv, (float)wr[c], acc[c]);
                }
            }
        }
    }
    sth_h* out = y + o * cout + co0;
    for (int c = 0; c < nco; c++) out[c] = (sth_h)acc[c];  // round to nearest even; overflow -> inf
}

// ------------------------------------------------------------------------------- forward, matrix form ---
// A wave = 16 output rows x CT column tiles of 16 channels (a workgroup: 4 waves, 64 rows; cout > 16 CT: column groups in the grid).
// Per offset and 32-channel chunk c: lane (i = l & 15, g = l >> 4) holds A[i][8g + e] = x[row i][32c + 8g + e] and
// B[8g + e][i] = W[k][32c + 8g + e][column i] (cdna_hip_programming.md section 3; channels past cin are zeros in both), and
// D[4g + r][i] = acc[r].  V8: the 8 channels of a lane are one 16-byte load (cin and c0 multiples of 8, aligned).
template <int CT, bool V8>
__global__ void __launch_bounds__(HC_BLOCK) k_hconv_mfma(const sth_h* __restrict__ x0, int c0, const sth_h* __restrict__ x1, int cin,
                                                         const int32_t* __restrict__ nbr, int K, int64_t n_out, int64_t nstride,
                                                         const sth_h* __restrict__ w, int cout, int co_groups, sth_h* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int cobase = (int)(blockIdx.x % (unsigned)co_groups) * (16 * CT);
    const int64_t obase = ((int64_t)(blockIdx.x / (unsigned)co_groups) * (HC_BLOCK / 64) + wave) * 16;
    const int64_t orow = obase + i16 < n_out ? obase + i16 : -1;
    const int c1 = cin - c0, nc = (cin + 31) / 32;
    const sth_h zero = (sth_h)0.0f;
    sth_v4f acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) acc[ct] = sth_v4f{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < K; k++) {
        const int idx = orow >= 0 ? (nbr ? nbr[(int64_t)k * nstride + orow] : (int)orow) : -1;
        if (__ballot(idx >= 0) == 0ull) continue;  // no row of this wave has a neighbour at offset k (wave-uniform)
        const sth_h* __restrict__ wk = w + (int64_t)k * cin * cout;
        for (int c = 0; c < nc; c++) {
            const int ci = 32 * c + 8 * g;
            sth_v8h a = sth_v8h{zero, zero, zero, zero, zero, zero, zero, zero};
            if (idx >= 0 && ci < cin) {
                if (V8) {
                    const sth_h* row = ci < c0 ? x0 + (int64_t)idx * c0 + ci : x1 + (int64_t)idx * c1 + (ci - c0);
                    a = *reinterpret_cast<const sth_v8h*>(row);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const int cc = ci + e;
                        if (cc < cin) a[e] = cc < c0 ? x0[(int64_t)idx * c0 + cc] : x1[(int64_t)idx * c1 + (cc - c0)];
                    }
                }
            }
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const int co = cobase + 16 * ct + i16;
                sth_v8h b = sth_v8h{zero, zero, zero, zero, zero, zero, zero, zero};
                if (co < cout) {
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        if (ci + e < cin) b[e] = wk[(int64_t)(ci + e) * cout + co];
                }
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[ct], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const int co = cobase + 16 * ct + i16;
        if (co >= cout) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t o = obase + 4 * g + r;
            if (o < n_out) y[o * cout + co] = (sth_h)acc[ct][r];
        }
    }
}

extern "C" int st_sparse_conv_h_fwd(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                    int64_t nbr_stride, const void* w, int cout, void* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(K >= 1 && (nbr != nullptr || K == 1), "conv(h): a NULL neighbour table means pointwise (K = 1)");
    ST_REQUIRE(c0 > 0 && c0 <= cin && (c0 == cin || x1 != nullptr), "conv(h): bad concat split");
    ST_REQUIRE(cout >= 1, "conv(h): cout must be positive");
    if (n_out <= 0) return ST_OK;
    ST_REQUIRE(x0 && w && y, "conv(h): null input");
    const int64_t nstride = nbr_stride > 0 ? nbr_stride : n_out;
    const uintptr_t addr = (uintptr_t)x0 | (uintptr_t)x1;
    const sth_h *hx0 = (const sth_h*)x0, *hx1 = (const sth_h*)x1, *hw = (const sth_h*)w;
    sth_h* hy = (sth_h*)y;
    if (hconv_matrix_form(cin, cout)) {
        const bool v8 = cin % 8 == 0 && c0 % 8 == 0 && (addr & 15) == 0;
        const int ct = cout <= 16 ? 1 : cout <= 32 ? 2 : cout <= 48 ? 3 : 4;
        const int groups = (int)st_div_up(cout, 16 * ct);
        const int64_t blocks = st_div_up(n_out, HC_BLOCK / 4) * groups;
#define HF_MFMA_CASE(CT_)                                                                                                              \
    if (ct == CT_) {                                                                                                                   \
        if (v8) hipLaunchKernelGGL((k_hconv_mfma<CT_, true>), dim3((unsigned)blocks), dim3(HC_BLOCK), 0, stream, hx0, c0, hx1, cin, nbr, \
                                   K, n_out, nstride, hw, cout, groups, hy);                                                          \
        else hipLaunchKernelGGL((k_hconv_mfma<CT_, false>), dim3((unsigned)blocks), dim3(HC_BLOCK), 0, stream, hx0, c0, hx1, cin, nbr, \
                                K, n_out, nstride, hw, cout, groups, hy);                                                             \
    }
        HF_MFMA_CASE(1)
        HF_MFMA_CASE(2)
        HF_MFMA_CASE(3)
        HF_MFMA_CASE(4)
#undef HF_MFMA_CASE
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    const bool v4 = cin % 4 == 0 && c0 % 4 == 0 && (addr & 7) == 0;
    const int cot = cout <= 4 ? 4 : 8;
    const int co_tiles = (int)st_div_up(cout, cot);
    const int64_t blocks = st_div_up(n_out, HC_BLOCK) * co_tiles;
#define HF_VEC_CASE(COT_)                                                                                                           \
    if (cot == COT_) {                                                                                                              \
        if (v4) hipLaunchKernelGGL((k_hconv_vec<COT_, true>), dim3((unsigned)blocks), dim3(HC_BLOCK), 0, stream, hx0, c0, hx1, cin, nbr, \
                                   K, n_out, nstride, hw, cout, co_tiles, hy);                                                       \
        else hipLaunchKernelGGL((k_hconv_vec<COT_, false>), dim3((unsigned)blocks), dim3(HC_BLOCK), 0, stream, hx0, c0, hx1, cin, nbr, \
                                K, n_out, nstride, hw, cout, co_tiles, hy);                                                          \
    }
    HF_VEC_CASE(4)
    HF_VEC_CASE(8)
#undef HF_VEC_CASE
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ------------------------------------------------------------------------------------- weight gradient ---
// Deterministic as st_sparse_conv_wgrad (csrc/sparse_conv_grad.hip), no float atomics:
//   pass 1  one workgroup per (tile group, offset k, row chunk): the chunk's live pairs of offset k are compacted in row order
//           (ballot + prefix over the workgroup) and staged through LDS as half in batches, then
//             matrix form  the live-pair axis is the MFMA's K: per 32 pairs, A[i][8g + e] = x[pair 8g + e][16ti + i],
//                          B[8g + e][i] = dy[pair 8g + e][16tj + i] and D = a 16 x 16 tile of dW[k] (pairs past the batch are zero rows
//                          in both operands).  A wave owns up to HW_MT tiles; a layer with fewer tiles than waves gives each tile G
//                          waves that take the batch's 32-pair blocks round-robin, and their sums are added in wave order;
//             vector form  every lane accumulates a 4 x 4 block of dW[k] with one fmaf per product (G lane groups share the pairs
//                          round-robin when the layer has fewer blocks than lanes, added in group order).
//           The partial sums go to a float32 slab per (chunk, k).
//   pass 2  one lane per weight adds the slabs in ascending chunk order.
// Row chunks: up to HW_MAX_CHUNKS per offset, a function of n_out only (four times the float32 kernel's count: a pointwise layer has
// one offset, and 64 chunks of a level-0-sized layer left most of the chip idle).
#define HW_BLOCK 256
#define HW_ROWS 256
#define HW_MAX_CHUNKS 256
#define HW_STAGE 16384  // halves of LDS for one batch of staged (input row, dy row) pairs
#define HW_TILE 256     // vector form: 4x4 blocks per workgroup
#define HW_MT 4         // matrix form: 16x16 tiles per wave (HW_MT * 4 per workgroup)

static inline int64_t hw_rows_per_chunk(int64_t n_out) {
    return (int64_t)HW_ROWS * st_div_up(st_div_up(n_out > 0 ? n_out : 1, HW_ROWS), HW_MAX_CHUNKS);
}
// the matrix form needs 32 staged pairs per batch
static inline bool hw_matrix_form(int cin, int cout) {
    return hconv_matrix_form(cin, cout) && ((cin + 15) & ~15) + ((cout + 15) & ~15) <= HW_STAGE / 32;
}

template <bool MF>
__global__ void __launch_bounds__(HW_BLOCK) k_hwgrad_partial(const sth_h* __restrict__ x0, int c0, const sth_h* __restrict__ x1, int cin,
                                                             const int32_t* __restrict__ nbr, int K, int64_t n_out, int64_t nstride,
                                                             const sth_h* __restrict__ dy, int cout, int64_t rows_per_chunk, int nchunks,
                                                             float* __restrict__ partial) {
    __shared__ int32_t s_idx[HW_ROWS];
    __shared__ int32_t s_row[HW_ROWS];  // output row - chunk start
    __shared__ int s_wcount[HW_BLOCK / 64];
    __shared__ float4 s_stage4[HW_STAGE / 8];
    sth_h* s_h = reinterpret_cast<sth_h*>(s_stage4);
    float* s_f = reinterpret_cast<float*>(s_stage4);  // the group reduce at the end (after the last batch)

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
    const int k = (int)((blockIdx.x / (unsigned)nchunks) % (unsigned)K);
    const int tg = (int)(blockIdx.x / ((unsigned)nchunks * (unsigned)K));
    const int c1 = cin - c0;
    const int q = MF ? 16 : 4;  // channel padding of a staged row
    const int cinp = (cin + q - 1) / q * q, coutp = (cout + q - 1) / q * q;
    int pb = HW_STAGE / (cinp + coutp) < HW_ROWS ? HW_STAGE / (cinp + coutp) : HW_ROWS;  // pairs per batch
    if (MF) pb &= ~31;
    sth_h* s_x = s_h;                // [pb][cinp]
    sth_h* s_dy = s_h + pb * cinp;   // [pb][coutp]
    const sth_h zero = (sth_h)0.0f;

    // matrix form: this workgroup's tiles tg * 4 HW_MT .. (at most), G waves per tile when there are fewer tiles than waves
    const int ntj = coutp / 16, ntiles = (cinp / 16) * ntj;
    const int mt0 = tg * HW_MT * (HW_BLOCK / 64);
    const int mtc = MF ? (ntiles - mt0 < HW_MT * (HW_BLOCK / 64) ? ntiles - mt0 : HW_MT * (HW_BLOCK / 64)) : 1;
    const int mG = mtc >= HW_BLOCK / 64 ? 1 : (HW_BLOCK / 64) / mtc;
    const int m_tile = mG == 1 ? wave : wave % mtc, m_grp = mG == 1 ? 0 : wave / mtc;
    const bool m_active = m_grp < mG;
    sth_v4f macc[HW_MT];
#pragma unroll
    for (int j = 0; j < HW_MT; j++) macc[j] = sth_v4f{0.0f, 0.0f, 0.0f, 0.0f};

    // vector form: 4x4 blocks
    const int cob = coutp / 4, nblk = (cinp / 4) * cob;
    const int tile_blk = nblk - tg * HW_TILE < HW_TILE ? nblk - tg * HW_TILE : HW_TILE;
    const int G = MF ? 1 : HW_BLOCK / tile_blk;
    const bool v_active = !MF && t < G * tile_blk;
    const int bl = MF ? 0 : t % tile_blk, vg = MF ? 0 : t / tile_blk;
    const int b = tg * HW_TILE + bl;
    const int ci0 = 4 * (b / cob), co0 = 4 * (b % cob);
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    const int64_t r_begin = (int64_t)chunk * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < n_out ? r_begin + rows_per_chunk : n_out;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += HW_ROWS) {
        const int64_t o = r0 + t;
        const int idx = o < r_end ? (nbr ? nbr[(int64_t)k * nstride + o] : (int)o) : -1;
        const unsigned long long m = __ballot(idx >= 0);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcount[wave] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
        for (int wv = 0; wv < HW_BLOCK / 64; wv++) {
            if (wv < wave) base += s_wcount[wv];
            total += s_wcount[wv];
        }
        if (idx >= 0) {
            s_idx[base + before] = idx;
            s_row[base + before] = (int32_t)(o - r_begin);
        }
        __syncthreads();
        for (int p0 = 0; p0 < total; p0 += pb) {
            const int np = total - p0 < pb ? total - p0 : pb;
            const int npp = MF ? (np + 31) & ~31 : np;  // staged rows (zero rows up to a 32-pair block)
            for (int e = t; e < npp * cinp; e += HW_BLOCK) {
                const int p = e / cinp, c = e - p * cinp;
                sth_h v = zero;
                if (p < np && c < cin) {
                    const int64_t i = s_idx[p0 + p];
                    v = c < c0 ? x0[i * c0 + c] : x1[i * c1 + (c - c0)];
                }
                s_x[e] = v;
            }
            for (int e = t; e < npp * coutp; e += HW_BLOCK) {
                const int p = e / coutp, c = e - p * coutp;
                s_dy[e] = p < np && c < cout ? dy[(r_begin + s_row[p0 + p]) * cout + c] : zero;
            }
            __syncthreads();
            if (MF) {
                if (m_active) {
                    const int i16 = lane & 15, g = lane >> 4;
                    for (int pblk = m_grp; pblk < npp / 32; pblk += mG) {
                        const int pr = 32 * pblk + 8 * g;
#pragma unroll
                        for (int j = 0; j < HW_MT; j++) {
                            const int tile = mt0 + m_tile + j * (HW_BLOCK / 64);
                            if (mG > 1 ? j > 0 : m_tile + j * (HW_BLOCK / 64) >= mtc) continue;  // wave-uniform
                            const int ti = tile / ntj, tj = tile - ti * ntj;
                            sth_v8h a, bv;
#pragma unroll
                            for (int e = 0; e < 8; e++) {
                                a[e] = s_x[(pr + e) * cinp + 16 * ti + i16];
                                bv[e] = s_dy[(pr + e) * coutp + 16 * tj + i16];
                            }
                            macc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv, macc[j], 0, 0, 0);
                        }
                    }
                }
            } else if (v_active) {
                for (int p = vg; p < np; p += G) {
                    const sth_v4h xv = *reinterpret_cast<const sth_v4h*>(s_x + p * cinp + ci0);
                    const sth_v4h dv = *reinterpret_cast<const sth_v4h*>(s_dy + p * coutp + co0);
                    const float xs[4] = {(float)xv.x, (float)xv.y, (float)xv.z, (float)xv.w};
                    const float ds[4] = {(float)dv.x, (float)dv.y, (float)dv.z, (float)dv.w};
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[4 * i + j] = fmaf(xs[i], ds[j], acc[4 * i + j]);
                }
            }
            __syncthreads();
        }
    }
    float* slab = partial + ((int64_t)chunk * K + k) * cin * cout;
    if (MF) {
        const int i16 = lane & 15, g = lane >> 4;
        if (mG > 1) {  // G waves per tile: their sums in wave-group order (mG * mtc <= 4 tiles of 256 floats)
            if (m_active) {
#pragma unroll
                for (int r = 0; r < 4; r++) s_f[((m_grp * mtc + m_tile) * 64 + lane) * 4 + r] = macc[0][r];
            }
            __syncthreads();
            if (m_active && m_grp == 0) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = s_f[(m_tile * 64 + lane) * 4 + r];
                    for (int q2 = 1; q2 < mG; q2++) v += s_f[((q2 * mtc + m_tile) * 64 + lane) * 4 + r];
                    macc[0][r] = v;
                }
            }
        }
        if (m_active && m_grp == 0) {
#pragma unroll
            for (int j = 0; j < HW_MT; j++) {
                if (mG > 1 ? j > 0 : m_tile + j * (HW_BLOCK / 64) >= mtc) continue;
                const int tile = mt0 + m_tile + j * (HW_BLOCK / 64);
                const int ti = tile / ntj, tj = tile - ti * ntj;
                const int co = 16 * tj + i16;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ci = 16 * ti + 4 * g + r;
                    if (ci < cin && co < cout) slab[ci * cout + co] = macc[j][r];
                }
            }
        }
        return;
    }
    // vector form: groups -> one sum per 4x4 block, in group order (G * tile_blk * 16 <= 4096 floats)
    if (v_active) {
#pragma unroll
        for (int e = 0; e < 16; e++) s_f[(vg * tile_blk + bl) * 16 + e] = acc[e];
    }
    __syncthreads();
    if (t < tile_blk) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            float v = s_f[bl * 16 + e];
            for (int q2 = 1; q2 < G; q2++) v += s_f[(q2 * tile_blk + bl) * 16 + e];
            const int ci = ci0 + (e >> 2), co = co0 + (e & 3);
            if (ci < cin && co < cout) slab[ci * cout + co] = v;
        }
    }
}

__global__ void __launch_bounds__(HW_BLOCK) k_hwgrad_reduce(const float* __restrict__ partial, int nchunks, int64_t n_w,
                                                            float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * HW_BLOCK + threadIdx.x;
    if (e >= n_w) return;
    float v = partial[e];
    for (int c = 1; c < nchunks; c++) v += partial[(int64_t)c * n_w + e];
    dw[e] = v;
}

extern "C" int64_t st_sparse_conv_wgrad_h_workspace_bytes(int K, int cin, int cout, int64_t n_out) {
    if (K < 1 || cin < 1 || cout < 1 || n_out < 0) return -1;
    const int64_t nchunks = st_div_up(n_out > 0 ? n_out : 1, hw_rows_per_chunk(n_out));
    return nchunks * K * cin * cout * (int64_t)sizeof(float) + 256;
}

extern "C" int st_sparse_conv_wgrad_h(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                      int64_t nbr_stride, const void* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(K >= 1 && cin >= 1 && cout >= 1 && n_out >= 0 && dw != nullptr, "wgrad(h): bad arguments");
    ST_REQUIRE(((cin + 3) & ~3) + ((cout + 3) & ~3) <= 8192, "wgrad(h): cin + cout > 8192");
    const int64_t n_w = (int64_t)K * cin * cout;
    if (n_out == 0) {  // (an empty table may come without storage)
        (void)hipMemsetAsync(dw, 0, n_w * sizeof(float), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    ST_REQUIRE(nbr != nullptr || K == 1, "wgrad(h): a NULL neighbour table means pointwise (K = 1)");
    ST_REQUIRE(c0 > 0 && c0 <= cin && (c0 == cin || x1 != nullptr), "wgrad(h): bad concat split");
    ST_REQUIRE(x0 && dy, "wgrad(h): null input");
    const int64_t need = st_sparse_conv_wgrad_h_workspace_bytes(K, cin, cout, n_out);
    if (ws == nullptr || ws_bytes < need) {
        st_set_error("wgrad(h): workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
        return ST_ERR_WORKSPACE;
    }
    const int64_t rows = hw_rows_per_chunk(n_out);
    const int nchunks = (int)st_div_up(n_out, rows);
    const int64_t nstride = nbr_stride > 0 ? nbr_stride : n_out;
    float* partial = (float*)ws;
    const sth_h *hx0 = (const sth_h*)x0, *hx1 = (const sth_h*)x1, *hdy = (const sth_h*)dy;
    const bool mf = hw_matrix_form(cin, cout);
    const int64_t groups = mf ? st_div_up(st_div_up(cin, 16) * st_div_up(cout, 16), HW_MT * (HW_BLOCK / 64))
                              : st_div_up(st_div_up(cin, 4) * st_div_up(cout, 4), HW_TILE);
    const int64_t blocks = groups * K * nchunks;
#define HW_FORM_CASE(MF_)                                                                                                          \
    if (mf == MF_)                                                                                                                 \
        hipLaunchKernelGGL((k_hwgrad_partial<MF_>), dim3((unsigned)blocks), dim3(HW_BLOCK), 0, stream, hx0, c0, hx1, cin, nbr, K, n_out, \
                           nstride, hdy, cout, rows, nchunks, partial);
    HW_FORM_CASE(true)
    HW_FORM_CASE(false)
#undef HW_FORM_CASE
    hipLaunchKernelGGL(k_hwgrad_reduce, dim3((unsigned)st_div_up(n_w, HW_BLOCK)), dim3(HW_BLOCK), 0, stream, (const float*)partial,
                       nchunks, n_w, dw);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ------------------------------------------------------------------------------------------- row moves ---
// dst[p] = src[order[p]] (scatter == 0) or dst[order[p]] = src[p] (scatter != 0) for rows of `row_elems` 2-byte elements (any count,
// odd included): st_move_rows for float16 features.
__global__ void __launch_bounds__(HC_BLOCK) k_move_rows_h(const uint16_t* __restrict__ src, int row_elems, const int32_t* __restrict__ order,
                                                          int64_t n, uint16_t* __restrict__ dst, int scatter) {
    const int64_t total = n * row_elems;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = t / row_elems;
        const int c = (int)(t - p * row_elems);
        const int64_t o = order[p];
        dst[(scatter ? o : p) * row_elems + c] = src[(scatter ? p : o) * row_elems + c];
    }
}

extern "C" int st_move_rows_h(const void* src, int row_elems, const int32_t* order, int64_t n, void* dst, int scatter, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0) return ST_OK;
    ST_REQUIRE(row_elems >= 1 && row_elems <= 512, "move_rows(h): rows of 1..512 elements");
    const int64_t blocks = st_div_up(n * row_elems, HC_BLOCK);
    hipLaunchKernelGGL(k_move_rows_h, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(HC_BLOCK), 0, stream, (const uint16_t*)src,
                       row_elems, order, n, (uint16_t*)dst, scatter);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
