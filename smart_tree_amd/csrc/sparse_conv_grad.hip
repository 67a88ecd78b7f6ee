// The weight gradient of a sparse convolution, for both storage types (training; the data gradient needs no kernel of its own, see
// smart_tree_amd/model/sparse_grad.py: it is the forward kernel over the transposed neighbour table with transposed weights).
//
//   dW[k][ci][co] = sum over o with nbr[k][o] >= 0 of cat(x0, x1)[nbr[k][o]][ci] * dY[o][co]
//
//   st_sparse_conv_wgrad     x0, x1, dY float32
//   st_sparse_conv_wgrad_h   x0, x1, dY IEEE half (float16 autocast); dW stays float32 and every sum is float32
//
// Replaces the weight-gradient half of spconv's backward (what autograd runs for SubMConv3d / SparseConv3d /
// SparseInverseConv3d when the reference trains, smart_tree/model/train.py:24-58, with and without fp16: True).
//
// One scheme, deterministic, no float atomics (cdna_hip_programming.md section 5, launch-boundary reduce):
//   pass 1  one workgroup per (tile group, offset k, row chunk): the chunk's live pairs of offset k are compacted in row order
//           (ballot + prefix over the workgroup) and staged through LDS in batches, in the storage type, then
//             vector form  every lane accumulates a 4 x 4 block of dW[k] with one fmaf per product.  Small layers have fewer blocks
//                          than lanes: then G groups of lanes take the batch's pairs round-robin (pair p -> group p % G) and the
//                          groups' sums are added in group order at the end;
//             matrix form  (half only) the live-pair axis is the MFMA's K: per 32 pairs, A[i][8g + e] = x[pair 8g + e][16ti + i],
//                          B[8g + e][i] = dy[pair 8g + e][16tj + i] and D = a 16 x 16 tile of dW[k] (pairs past the batch are zero rows
//                          in both operands).  A wave owns up to HW_MT tiles; a layer with fewer tiles than waves gives each tile G
//                          waves that take the batch's 32-pair blocks round-robin, and their sums are added in wave order.
//           The partial sums go to a float32 slab per (chunk, k) in the workspace.
//   pass 2  one lane per weight adds the slabs in ascending chunk order.
// The chunking depends on n_out only, the group count on (cin, cout) only: two calls give the same bits.  A product of two halves is
// exact in float32, so on the vector form half inputs give the bits of the float32 kernel on the same values.  Nothing clamps: an
// inf / NaN operand reaches every sum it takes part in.
#include <type_traits>

#include "st_common.h"

typedef _Float16 wg_v8h __attribute__((ext_vector_type(8)));
typedef float wg_v4f __attribute__((ext_vector_type(4)));

#define WG_BLOCK 256
#define WG_ROWS 256            // rows compacted per step (one per lane)
#define WG_STAGE_BYTES 32768   // LDS for one batch of staged (input row, dY row) pairs
#define HW_TILE 256            // vector form: 4x4 blocks per workgroup (one per lane when the layer has that many)
#define HW_MT 4                // matrix form: 16x16 tiles per wave (HW_MT * 4 per workgroup)

// What differs between the storage types.  max_chunks, the row chunks per offset, bounds the workspace and pass 2's length: for
// float32 256 measured slower in total (profiles/r07_bench_train.json); half takes four times as many (a pointwise layer has one
// offset, and 64 chunks of a level-0-sized layer left most of the chip idle).
template <typename T>
struct WgradPolicy;
template <>
struct WgradPolicy<float> {
    static constexpr int max_chunks = 64;
    static constexpr bool matrix_form = false;
    static constexpr const char* name = "wgrad";
};
template <>
struct WgradPolicy<_Float16> {
    static constexpr int max_chunks = 256;
    static constexpr bool matrix_form = true;
    static constexpr const char* name = "wgrad(h)";
};

template <typename T>
constexpr int wg_stage = WG_STAGE_BYTES / (int)sizeof(T);  // staged elements per batch

template <typename T>
static inline int64_t wg_rows_per_chunk(int64_t n_out) {
    return (int64_t)WG_ROWS * st_div_up(st_div_up(n_out > 0 ? n_out : 1, WG_ROWS), WgradPolicy<T>::max_chunks);
}
// Which form a (cin, cout) takes: the matrix form from 16 channels on both sides (as the half forward, hconv_matrix_form of
// sparse_conv_half.hip), while 32 staged pairs fit a batch.
template <typename T>
static inline bool wg_matrix_form(int cin, int cout) {
    return WgradPolicy<T>::matrix_form && cin >= 16 && cout >= 16 && ((cin + 15) & ~15) + ((cout + 15) & ~15) <= wg_stage<T> / 32;
}

template <typename T, bool MF>
__device__ __forceinline__ void wgrad_partial(const T* __restrict__ x0, int c0, const T* __restrict__ x1, int cin,
                                              const int32_t* __restrict__ nbr, int K, int64_t n_out, int64_t nstride,
                                              const T* __restrict__ dy, int cout, int64_t rows_per_chunk, int nchunks,
                                              float* __restrict__ partial) {
    static_assert(!MF || std::is_same<T, _Float16>::value, "the matrix form is the half policy's");
    typedef T v4t __attribute__((ext_vector_type(4)));
    __shared__ int32_t s_idx[WG_ROWS];
    __shared__ int32_t s_row[WG_ROWS];  // output row - chunk start
    __shared__ int s_wcount[WG_BLOCK / 64];
    __shared__ float4 s_stage4[WG_STAGE_BYTES / 16];
    T* s_t = reinterpret_cast<T*>(s_stage4);
    float* s_f = reinterpret_cast<float*>(s_stage4);  // the group reduce at the end (after the last batch)

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
    const int k = (int)((blockIdx.x / (unsigned)nchunks) % (unsigned)K);
    const int tg = (int)(blockIdx.x / ((unsigned)nchunks * (unsigned)K));
    const int c1 = cin - c0;
    constexpr int q = MF ? 16 : 4;  // channel padding of a staged row
    const int cinp = (cin + q - 1) / q * q, coutp = (cout + q - 1) / q * q;
    int pb = wg_stage<T> / (cinp + coutp) < WG_ROWS ? wg_stage<T> / (cinp + coutp) : WG_ROWS;  // pairs per batch
    if constexpr (MF) pb &= ~31;
    T* s_x = s_t;               // [pb][cinp]
    T* s_dy = s_t + pb * cinp;  // [pb][coutp]
    const T zero = (T)0.0f;
    const int64_t r_begin = (int64_t)chunk * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < n_out ? r_begin + rows_per_chunk : n_out;
    float* slab = partial + ((int64_t)chunk * K + k) * cin * cout;

    // the chunk's live pairs, batch by batch: accumulate(np, npp) sees np staged pairs in s_x / s_dy (npp rows with the zero rows)
    auto for_each_batch = [&](auto accumulate) {
        for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_ROWS) {
            const int64_t o = r0 + t;
            const int idx = o < r_end ? (nbr ? nbr[(int64_t)k * nstride + o] : (int)o) : -1;
            const unsigned long long m = __ballot(idx >= 0);
            const int before = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) s_wcount[wave] = __popcll(m);
            __syncthreads();
            int base = 0, total = 0;
            for (int wv = 0; wv < WG_BLOCK / 64; wv++) {
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
                for (int e = t; e < npp * cinp; e += WG_BLOCK) {
                    const int p = e / cinp, c = e - p * cinp;
                    T v = zero;
                    if ((!MF || p < np) && c < cin) {
                        const int64_t i = s_idx[p0 + p];
                        v = c < c0 ? x0[i * c0 + c] : x1[i * c1 + (c - c0)];
                    }
                    s_x[e] = v;
                }
                for (int e = t; e < npp * coutp; e += WG_BLOCK) {
                    const int p = e / coutp, c = e - p * coutp;
                    s_dy[e] = (!MF || p < np) && c < cout ? dy[(r_begin + s_row[p0 + p]) * cout + c] : zero;
                }
                __syncthreads();
                accumulate(np, npp);
                __syncthreads();
            }
        }
    };

    if constexpr (MF) {
        // this workgroup's tiles tg * 4 HW_MT .. (at most), G waves per tile when there are fewer tiles than waves
        const int ntj = coutp / 16, ntiles = (cinp / 16) * ntj;
        const int mt0 = tg * HW_MT * (WG_BLOCK / 64);
        const int mtc = ntiles - mt0 < HW_MT * (WG_BLOCK / 64) ? ntiles - mt0 : HW_MT * (WG_BLOCK / 64);
        const int mG = mtc >= WG_BLOCK / 64 ? 1 : (WG_BLOCK / 64) / mtc;
        const int m_tile = mG == 1 ? wave : wave % mtc, m_grp = mG == 1 ? 0 : wave / mtc;
        const bool m_active = m_grp < mG;
        const int i16 = lane & 15, g = lane >> 4;
        wg_v4f macc[HW_MT];
#pragma unroll
        for (int j = 0; j < HW_MT; j++) macc[j] = wg_v4f{0.0f, 0.0f, 0.0f, 0.0f};
        for_each_batch([&](int, int npp) {
            if (!m_active) return;
            for (int pblk = m_grp; pblk < npp / 32; pblk += mG) {
                const int pr = 32 * pblk + 8 * g;
#pragma unroll
                for (int j = 0; j < HW_MT; j++) {
                    const int tile = mt0 + m_tile + j * (WG_BLOCK / 64);
                    if (mG > 1 ? j > 0 : m_tile + j * (WG_BLOCK / 64) >= mtc) continue;  // wave-uniform
                    const int ti = tile / ntj, tj = tile - ti * ntj;
                    wg_v8h a, bv;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        a[e] = s_x[(pr + e) * cinp + 16 * ti + i16];
                        bv[e] = s_dy[(pr + e) * coutp + 16 * tj + i16];
                    }
                    macc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv, macc[j], 0, 0, 0);
                }
            }
        });
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
                if (mG > 1 ? j > 0 : m_tile + j * (WG_BLOCK / 64) >= mtc) continue;
                const int tile = mt0 + m_tile + j * (WG_BLOCK / 64);
                const int ti = tile / ntj, tj = tile - ti * ntj;
                const int co = 16 * tj + i16;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ci = 16 * ti + 4 * g + r;
                    if (ci < cin && co < cout) slab[ci * cout + co] = macc[j][r];
                }
            }
        }
    } else {
        const int cob = coutp / 4, nblk = (cinp / 4) * cob;
        const int tile_blk = nblk - tg * HW_TILE < HW_TILE ? nblk - tg * HW_TILE : HW_TILE;
        const int G = WG_BLOCK / tile_blk;  // lane groups sharing a batch's pairs
        const bool active = t < G * tile_blk;
        const int bl = t % tile_blk, vg = t / tile_blk;
        const int b = tg * HW_TILE + bl;
        const int ci0 = 4 * (b / cob), co0 = 4 * (b % cob);
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] = 0.0f;
        for_each_batch([&](int np, int) {
            if (!active) return;
            for (int p = vg; p < np; p += G) {
                const v4t xv = *reinterpret_cast<const v4t*>(s_x + p * cinp + ci0);
                const v4t dv = *reinterpret_cast<const v4t*>(s_dy + p * coutp + co0);
                const float xs[4] = {(float)xv.x, (float)xv.y, (float)xv.z, (float)xv.w};
                const float ds[4] = {(float)dv.x, (float)dv.y, (float)dv.z, (float)dv.w};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[4 * i + j] = fmaf(xs[i], ds[j], acc[4 * i + j]);
            }
        });
        // groups -> one sum per 4x4 block, in group order (G * tile_blk * 16 <= 4096 floats: the staging buffer is free again)
        if (active) {
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
}

// one kernel name per storage type and form
#define WG_KERNEL_ARGS(T)                                                                                                        \
    const T *__restrict__ x0, int c0, const T *__restrict__ x1, int cin, const int32_t *__restrict__ nbr, int K, int64_t n_out, \
        int64_t nstride, const T *__restrict__ dy, int cout, int64_t rows_per_chunk, int nchunks, float *__restrict__ partial
#define WG_KERNEL_PASS x0, c0, x1, cin, nbr, K, n_out, nstride, dy, cout, rows_per_chunk, nchunks, partial

__global__ void __launch_bounds__(WG_BLOCK) k_wgrad_partial(WG_KERNEL_ARGS(float)) { wgrad_partial<float, false>(WG_KERNEL_PASS); }

template <bool MF>
__global__ void __launch_bounds__(WG_BLOCK) k_hwgrad_partial(WG_KERNEL_ARGS(_Float16)) {
    wgrad_partial<_Float16, MF>(WG_KERNEL_PASS);
}

__global__ void __launch_bounds__(WG_BLOCK) k_wgrad_reduce(const float* __restrict__ partial, int nchunks, int64_t n_w,
                                                           float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (e >= n_w) return;
    float v = partial[e];
    for (int c = 1; c < nchunks; c++) v += partial[(int64_t)c * n_w + e];
    dw[e] = v;
}

template <typename T>
static int64_t wgrad_ws_bytes(int K, int cin, int cout, int64_t n_out) {
    if (K < 1 || cin < 1 || cout < 1 || n_out < 0) return -1;
    const int64_t nchunks = st_div_up(n_out > 0 ? n_out : 1, wg_rows_per_chunk<T>(n_out));
    return nchunks * K * cin * cout * (int64_t)sizeof(float) + 256;
}

template <typename T>
static int wgrad_run(const T* x0, int c0, const T* x1, int cin, const int32_t* nbr, int K, int64_t n_out, int64_t nbr_stride,
                     const T* dy, int cout, float* dw, void* ws, int64_t ws_bytes, hipStream_t stream) {
    const char* name = WgradPolicy<T>::name;
    ST_REQUIRE(K >= 1 && cin >= 1 && cout >= 1 && n_out >= 0 && dw != nullptr, "%s: bad arguments", name);
    ST_REQUIRE(((cin + 3) & ~3) + ((cout + 3) & ~3) <= 8192, "%s: cin + cout > 8192", name);
    const int64_t n_w = (int64_t)K * cin * cout;
    if (n_out == 0) {  // (an empty table may come without storage)
        (void)hipMemsetAsync(dw, 0, n_w * sizeof(float), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    ST_REQUIRE(nbr != nullptr || K == 1, "%s: a NULL neighbour table means pointwise (K = 1)", name);
    ST_REQUIRE(c0 > 0 && c0 <= cin && (c0 == cin || x1 != nullptr), "%s: bad concat split", name);
    ST_REQUIRE(x0 && dy, "%s: null input", name);
    const int64_t need = wgrad_ws_bytes<T>(K, cin, cout, n_out);
    if (ws == nullptr || ws_bytes < need) {
        st_set_error("%s: workspace too small (%lld < %lld)", name, (long long)ws_bytes, (long long)need);
        return ST_ERR_WORKSPACE;
    }
    const int64_t rows_per_chunk = wg_rows_per_chunk<T>(n_out);
    const int nchunks = (int)st_div_up(n_out, rows_per_chunk);
    const int64_t nstride = nbr_stride > 0 ? nbr_stride : n_out;
    float* partial = (float*)ws;
    const bool mf = wg_matrix_form<T>(cin, cout);
    const int64_t groups = mf ? st_div_up(st_div_up(cin, 16) * st_div_up(cout, 16), HW_MT * (WG_BLOCK / 64))
                              : st_div_up(st_div_up(cin, 4) * st_div_up(cout, 4), HW_TILE);
    const dim3 grid((unsigned)(groups * K * nchunks)), block(WG_BLOCK);
    if constexpr (std::is_same<T, float>::value) {
        hipLaunchKernelGGL(k_wgrad_partial, grid, block, 0, stream, WG_KERNEL_PASS);
    } else {
#define HW_FORM_CASE(MF_) \
    if (mf == MF_) hipLaunchKernelGGL((k_hwgrad_partial<MF_>), grid, block, 0, stream, WG_KERNEL_PASS);
        HW_FORM_CASE(true)
        HW_FORM_CASE(false)
#undef HW_FORM_CASE
    }
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)st_div_up(n_w, WG_BLOCK)), block, 0, stream, (const float*)partial, nchunks, n_w,
                       dw);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int64_t st_sparse_conv_wgrad_workspace_bytes(int K, int cin, int cout, int64_t n_out) {
    return wgrad_ws_bytes<float>(K, cin, cout, n_out);
}
extern "C" int64_t st_sparse_conv_wgrad_h_workspace_bytes(int K, int cin, int cout, int64_t n_out) {
    return wgrad_ws_bytes<_Float16>(K, cin, cout, n_out);
}
extern "C" int st_sparse_conv_wgrad(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                    int64_t nbr_stride, const float* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream) {
    return wgrad_run<float>(x0, c0, x1, cin, nbr, K, n_out, nbr_stride, dy, cout, dw, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int st_sparse_conv_wgrad_h(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                      int64_t nbr_stride, const void* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream) {
    return wgrad_run<_Float16>((const _Float16*)x0, c0, (const _Float16*)x1, cin, nbr, K, n_out, nbr_stride, (const _Float16*)dy, cout, dw,
                               ws, ws_bytes, (hipStream_t)stream);
}
