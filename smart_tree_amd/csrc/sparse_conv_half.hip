// Half-precision sparse convolution for mixed-precision (autocast float16) training:
//
//   st_sparse_conv_h_fwd     y[o] = sum_k cat(x0, x1)[nbr[k][o]] . W[k]     x0, x1, W [K][cin][cout], y: IEEE half
//   st_move_rows_h           rows of 2-byte elements moved by a permutation (the spatial order into / out of the network)
//
// The data gradient is st_sparse_conv_h_fwd over the transposed table with transposed weights (model/sparse_grad.py); the weight
// gradient of half features, st_sparse_conv_wgrad_h, is the half policy of the one weight-gradient body in sparse_conv_grad.hip.
// Replaces what spconv's SubMConv3d / SparseConv3d / SparseInverseConv3d run forward when the reference trains under
// torch.cuda.amp.autocast (smart_tree/model/train.py:24-58, conf/training.yaml fp16: True).
//
// Arithmetic: products of two halves are exact in float32; every sum is float32 (fmaf chains on the vector form,
// v_mfma_f32_16x16x32_f16 on the matrix form); the forward rounds once to half at the store.
// Nothing clamps: an inf / NaN operand reaches every sum it takes part in (loss scaling needs an overflowed dy to show up in dx).
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

typedef void (*hconv_kernel_t)(const sth_h*, int, const sth_h*, int, const int32_t*, int, int64_t, int64_t, const sth_h*, int, int, sth_h*);

extern "C" int st_sparse_conv_h_fwd(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                    int64_t nbr_stride, const void* w, int cout, void* y, void* stream_) {
    ST_REQUIRE(K >= 1 && (nbr != nullptr || K == 1), "conv(h): a NULL neighbour table means pointwise (K = 1)");
    ST_REQUIRE(c0 > 0 && c0 <= cin && (c0 == cin || x1 != nullptr), "conv(h): bad concat split");
    ST_REQUIRE(cout >= 1, "conv(h): cout must be positive");
    if (n_out <= 0) return ST_OK;
    ST_REQUIRE(x0 && w && y, "conv(h): null input");
    const int64_t nstride = nbr_stride > 0 ? nbr_stride : n_out;
    // both forms' kernels take the same arguments; tiles = column tiles (vector form) or column groups (matrix form) in the grid
    auto launch = [&](hconv_kernel_t kernel, int64_t blocks, int tiles) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(HC_BLOCK), 0, (hipStream_t)stream_, (const sth_h*)x0, c0, (const sth_h*)x1,
                           cin, nbr, K, n_out, nstride, (const sth_h*)w, cout, tiles, (sth_h*)y);
    };
    const uintptr_t addr = (uintptr_t)x0 | (uintptr_t)x1;
    if (hconv_matrix_form(cin, cout)) {
        const bool v8 = cin % 8 == 0 && c0 % 8 == 0 && (addr & 15) == 0;
        const int ct = cout <= 16 ? 1 : cout <= 32 ? 2 : cout <= 48 ? 3 : 4;
        const int groups = (int)st_div_up(cout, 16 * ct);
        const int64_t blocks = st_div_up(n_out, HC_BLOCK / 4) * groups;
#define HF_MFMA_CASE(CT_) \
    if (ct == CT_) launch(v8 ? k_hconv_mfma<CT_, true> : k_hconv_mfma<CT_, false>, blocks, groups);
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
#define HF_VEC_CASE(COT_) \
    if (cot == COT_) launch(v4 ? k_hconv_vec<COT_, true> : k_hconv_vec<COT_, false>, blocks, co_tiles);
    HF_VEC_CASE(4)
    HF_VEC_CASE(8)
#undef HF_VEC_CASE
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
