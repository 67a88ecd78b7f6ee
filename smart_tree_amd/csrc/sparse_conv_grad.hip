// st_sparse_conv_wgrad: the weight gradient of a sparse convolution (training; the data gradient needs no kernel of its own, see
// smart_tree_amd/model/sparse_grad.py: it is st_sparse_conv_fwd over the transposed neighbour table with transposed weights).
//
//   dW[k][ci][co] = sum over o with nbr[k][o] >= 0 of cat(x0, x1)[nbr[k][o]][ci] * dY[o][co]
//
// Replaces the weight-gradient half of spconv's backward (what autograd runs for SubMConv3d / SparseConv3d /
// SparseInverseConv3d when the reference trains, smart_tree/model/train.py:24-58).
//
// Deterministic, no float atomics (cdna_hip_programming.md section 5, launch-boundary reduce):
//   pass 1  one workgroup per (4x4-block tile, offset k, row chunk): the chunk's live pairs of offset k are compacted in row order
//           (ballot + prefix over the workgroup), staged through LDS in batches, and every lane accumulates a 4x4 block of dW[k]
//           with one fmaf per product.  Small layers have fewer 4x4 blocks than lanes: then G groups of lanes take the batch's
//           pairs round-robin (pair p -> group p % G) and the groups' sums are added in group order at the end.  The partial
//           sums go to a slab per (chunk, k) in the workspace.
//   pass 2  one lane per weight adds the slabs in ascending chunk order.
// The chunking depends on n_out only, the group count on (cin, cout) only: two calls give the same bits.
#include "st_common.h"

#define WG_BLOCK 256
#define WG_ROWS 256        // rows compacted per step (one per lane)
#define WG_MAX_CHUNKS 64   // row chunks per offset: bounds the workspace and pass 2's length (256 measured slower in total: profiles/r07_bench_train.json)
#define WG_STAGE 8192      // floats of LDS for one batch of staged (input row, dY row) pairs
#define WG_TILE 256        // 4x4 blocks per workgroup (one per lane when the layer has that many)

static inline int64_t wg_rows_per_chunk(int64_t n_out) {
    return (int64_t)WG_ROWS * st_div_up(st_div_up(n_out > 0 ? n_out : 1, WG_ROWS), WG_MAX_CHUNKS);
}

__global__ void __launch_bounds__(WG_BLOCK) k_wgrad_partial(const float* __restrict__ x0, int c0, const float* __restrict__ x1, int cin,
                                                            const int32_t* __restrict__ nbr, int K, int64_t n_out, int64_t nstride,
                                                            const float* __restrict__ dy, int cout, int64_t rows_per_chunk, int nchunks,
                                                            float* __restrict__ partial) {
    __shared__ int32_t s_idx[WG_ROWS];
    __shared__ int32_t s_row[WG_ROWS];  // output row - chunk start
    __shared__ int s_wcount[WG_BLOCK / 64];
    __shared__ float4 s_stage4[WG_STAGE / 4];
    float* s_stage = reinterpret_cast<float*>(s_stage4);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
    const int k = (int)((blockIdx.x / (unsigned)nchunks) % (unsigned)K);
    const int tile = (int)(blockIdx.x / ((unsigned)nchunks * (unsigned)K));
    const int cin4 = (cin + 3) & ~3, cout4 = (cout + 3) & ~3, c1 = cin - c0;
    const int cob = cout4 / 4, nblk = (cin4 / 4) * cob;
    const int tile_blk = nblk - tile * WG_TILE < WG_TILE ? nblk - tile * WG_TILE : WG_TILE;
    const int G = WG_BLOCK / tile_blk;  // lane groups sharing a batch's pairs
    const bool active = t < G * tile_blk;
    const int bl = t % tile_blk, g = t / tile_blk;
    const int b = tile * WG_TILE + bl;
    const int ci0 = 4 * (b / cob), co0 = 4 * (b % cob);
    const int pb = WG_STAGE / (cin4 + cout4) < WG_ROWS ? WG_STAGE / (cin4 + cout4) : WG_ROWS;  // pairs per batch
    float* s_x = s_stage;               // [pb][cin4]
    float* s_dy = s_stage + pb * cin4;  // [pb][cout4]

    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    const int64_t r_begin = (int64_t)chunk * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < n_out ? r_begin + rows_per_chunk : n_out;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_ROWS) {
        const int64_t o = r0 + t;
        const int idx = o < r_end ? (nbr ? nbr[(int64_t)k * nstride + o] : (int)o) : -1;
        const unsigned long long m = __ballot(idx >= 0);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcount[wave] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < WG_BLOCK / 64; w++) {
            if (w < wave) base += s_wcount[w];
            total += s_wcount[w];
        }
        if (idx >= 0) {
            s_idx[base + before] = idx;
            s_row[base + before] = (int32_t)(o - r_begin);
        }
        __syncthreads();
        for (int p0 = 0; p0 < total; p0 += pb) {
            const int np = total - p0 < pb ? total - p0 : pb;
            for (int e = t; e < np * cin4; e += WG_BLOCK) {
                const int p = e / cin4, c = e - p * cin4;
                const int64_t i = s_idx[p0 + p];
                s_x[e] = c < c0 ? x0[i * c0 + c] : (c < cin ? x1[i * c1 + (c - c0)] : 0.0f);
            }
            for (int e = t; e < np * cout4; e += WG_BLOCK) {
                const int p = e / cout4, c = e - p * cout4;
                s_dy[e] = c < cout ? dy[(r_begin + s_row[p0 + p]) * cout + c] : 0.0f;
            }
            __syncthreads();
            if (active) {
                for (int p = g; p < np; p += G) {
                    const float4 xv = *reinterpret_cast<const float4*>(s_x + p * cin4 + ci0);
                    const float4 dv = *reinterpret_cast<const float4*>(s_dy + p * cout4 + co0);
                    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[4 * i + j] = fmaf(xs[i], ds[j], acc[4 * i + j]);
                }
            }
            __syncthreads();
        }
    }
    // groups -> one sum per 4x4 block, in group order (G * tile_blk * 16 <= 4096 floats: the staging buffer is free again)
    if (active) {
#pragma unroll
        for (int e = 0; e < 16; e++) s_stage[(g * tile_blk + bl) * 16 + e] = acc[e];
    }
    __syncthreads();
    if (t < tile_blk) {
        float* slab = partial + ((int64_t)chunk * K + k) * cin * cout;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            float v = s_stage[bl * 16 + e];
            for (int q = 1; q < G; q++) v += s_stage[(q * tile_blk + bl) * 16 + e];
            const int ci = ci0 + (e >> 2), co = co0 + (e & 3);
            if (ci < cin && co < cout) slab[ci * cout + co] = v;
        }
    }
}

__global__ void __launch_bounds__(WG_BLOCK) k_wgrad_reduce(const float* __restrict__ partial, int nchunks, int64_t n_w,
                                                           float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (e >= n_w) return;
    float v = partial[e];
    for (int c = 1; c < nchunks; c++) v += partial[(int64_t)c * n_w + e];
    dw[e] = v;
}

extern "C" int64_t st_sparse_conv_wgrad_workspace_bytes(int K, int cin, int cout, int64_t n_out) {
    if (K < 1 || cin < 1 || cout < 1 || n_out < 0) return -1;
    const int64_t nchunks = st_div_up(n_out > 0 ? n_out : 1, wg_rows_per_chunk(n_out));
    return nchunks * K * cin * cout * (int64_t)sizeof(float) + 256;
}

extern "C" int st_sparse_conv_wgrad(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                    int64_t nbr_stride, const float* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(K >= 1 && cin >= 1 && cout >= 1 && n_out >= 0 && dw != nullptr, "wgrad: bad arguments");
    ST_REQUIRE(((cin + 3) & ~3) + ((cout + 3) & ~3) <= WG_STAGE, "wgrad: cin + cout > %d", WG_STAGE);
    const int64_t n_w = (int64_t)K * cin * cout;
    if (n_out == 0) {  // (an empty table may come without storage)
        (void)hipMemsetAsync(dw, 0, n_w * sizeof(float), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    ST_REQUIRE(nbr != nullptr || K == 1, "wgrad: a NULL neighbour table means pointwise (K = 1)");
    ST_REQUIRE(c0 > 0 && c0 <= cin && (c0 == cin || x1 != nullptr), "wgrad: bad concat split");
    ST_REQUIRE(x0 && dy, "wgrad: null input");
    const int64_t need = st_sparse_conv_wgrad_workspace_bytes(K, cin, cout, n_out);
    if (ws == nullptr || ws_bytes < need) {
        st_set_error("wgrad: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
        return ST_ERR_WORKSPACE;
    }
    const int64_t rows = wg_rows_per_chunk(n_out);
    const int nchunks = (int)st_div_up(n_out, rows);
    const int64_t nblk = (int64_t)((cin + 3) / 4) * ((cout + 3) / 4);
    const int64_t blocks = st_div_up(nblk, WG_TILE) * K * nchunks;
    const int64_t nstride = nbr_stride > 0 ? nbr_stride : n_out;
    float* partial = (float*)ws;
    hipLaunchKernelGGL(k_wgrad_partial, dim3((unsigned)blocks), dim3(WG_BLOCK), 0, stream, x0, c0, x1, cin, nbr, K, n_out, nstride, dy,
                       cout, rows, nchunks, partial);
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)st_div_up(n_w, WG_BLOCK)), dim3(WG_BLOCK), 0, stream, (const float*)partial,
                       nchunks, n_w, dw);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
