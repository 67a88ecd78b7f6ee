// Training-mode BatchNorm over [n, C] rows, in four passes a synchronised BatchNorm (model/sync_bn.py) interleaves with its two
// all-reduces:
//
//   st_bn_stats            out = [sum x | sum x^2 | n] per channel, float64                       (forward, before the all-reduce)
//   st_bn_apply            y = (x - mean) * invstd * gamma + beta                                  (forward, after it)
//   st_bn_backward_stats   out = [sum dy | sum dy * xhat] per channel, float64, xhat = (x - mean) * invstd recomputed from x
//   st_bn_backward_apply   dx = gamma * invstd * (dy - sum_dy / N - xhat * sum_dy_xhat / N), N = the global row count
//
// Replaces torch.nn.BatchNorm1d's training forward and backward (eps and momentum are the caller's), as the reference's
// model_blocks.py uses it, with the batch statistics taken over every rank's rows instead of one process's.
// Every form takes float32 or IEEE half x / dy / y / dx (`half`); mean, invstd, gamma, beta are float32 and the arithmetic is
// float32 per element, float64 in the sums -- what BatchNorm does on half input under autocast.
//
// Determinism: no float atomics.  The rows are cut into chunks whose size depends on (n, C) alone; a workgroup sums one chunk
// (lane -> LDS in row order), a second launch adds the chunk partials in a fixed order (lane l takes chunks l, l + 64, ...,
// then a fixed shuffle tree).  Two calls give the same bits.
//
// Mapping: a workgroup of 256 lanes covers a tile of up to 256 channels (blockIdx.y) and 256 / width rows at a time; each lane
// keeps one channel, so consecutive lanes read consecutive addresses of a row-major [n, C] array.
#include "st_common.h"

typedef _Float16 stbn_h;

#define BN_BLOCK 256
#define BN_TILE 256            // channels per workgroup column
#define BN_CHUNK_ELEMS 8192    // elements per stats chunk (at least): 32 per lane
#define BN_MAX_CHUNKS 1024     // chunk count cap: above it chunks grow (about 1M rows x 8 channels reaches it)
#define BN_MAX_C 4096
#define BN_APPLY_ROWS_PER_LANE 4
#define BN_APPLY_MAX_BLOCKS 2048

static inline int64_t bn_rows_per_chunk(int64_t n, int C) {
    const int64_t by_size = st_div_up(BN_CHUNK_ELEMS, C);
    const int64_t by_cap = st_div_up(n > 0 ? n : 1, BN_MAX_CHUNKS);
    return by_size > by_cap ? by_size : by_cap;
}

static inline int64_t bn_chunks(int64_t n, int C) { return st_div_up(n > 0 ? n : 1, bn_rows_per_chunk(n, C)); }

template <class T>
__device__ __forceinline__ float bn_load(const T* p, int64_t i) { return (float)p[i]; }

// MODE 0: (sum x, sum x^2); MODE 1: (sum dy, sum dy * xhat).  partial is [nchunks][2C]: the first C entries of a chunk's row are
// the first sums, the next C the second.
template <class T, int MODE>
__global__ void __launch_bounds__(BN_BLOCK) k_bn_partial(const T* __restrict__ x, const T* __restrict__ dy, int64_t n, int C,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         int64_t rows_per_chunk, double* __restrict__ partial) {
    __shared__ double sa[BN_BLOCK];
    __shared__ double sb[BN_BLOCK];
    const int c0 = (int)blockIdx.y * BN_TILE;
    const int width = C - c0 < BN_TILE ? C - c0 : BN_TILE;
    const int R = BN_BLOCK / width;  // rows per step
    const int t = threadIdx.x;
    const int c = t % width, rr = t / width;
    const int col = c0 + c;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
    double a = 0.0, b = 0.0;
    if (rr < R) {
        float m = 0.0f, s = 0.0f;
        if (MODE == 1) { m = mean[col]; s = invstd[col]; }
        for (int64_t r = r0 + rr; r < r1; r += R) {
            const float v = bn_load(x, r * C + col);
            if (MODE == 0) {
                a += (double)v;
                b += (double)v * (double)v;
            } else {
                const float g = bn_load(dy, r * C + col);
                const float xh = (v - m) * s;
                a += (double)g;
                b += (double)g * (double)xh;
            }
        }
    }
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    if (t < width) {
        double A = 0.0, B = 0.0;
        for (int k = 0; k < R; k++) {
            A += sa[k * width + t];
            B += sb[k * width + t];
        }
        double* row = partial + (int64_t)blockIdx.x * 2 * C;
        row[col] = A;
        row[C + col] = B;
    }
}

// One wave per output entry j < 2C: lane l adds chunks l, l + 64, ... in order, then a fixed xor tree.  MODE 0 appends n.
__global__ void __launch_bounds__(BN_BLOCK) k_bn_final(const double* __restrict__ partial, int nchunks, int C, int64_t n, int mode,
                                                       double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t m = 2 * (int64_t)C;
    double v = 0.0;
    if (j < m)
        for (int k = lane; k < nchunks; k += 64) v += partial[(int64_t)k * m + j];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if (j < m && lane == 0) out[j] = v;
    if (mode == 0 && blockIdx.x == 0 && threadIdx.x == 0) out[m] = (double)n;
}

// MODE 0: y = (x - mean) * invstd * gamma + beta.  MODE 1: dx = gamma * invstd * (dy - sum_dy / N - xhat * sum_dy_xhat / N).
template <class T, int MODE>
__global__ void __launch_bounds__(BN_BLOCK) k_bn_apply(const T* __restrict__ x, const T* __restrict__ dy, int64_t n, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const double* __restrict__ sums, const double* __restrict__ count,
                                                       T* __restrict__ out) {
    const int c0 = (int)blockIdx.y * BN_TILE;
    const int width = C - c0 < BN_TILE ? C - c0 : BN_TILE;
    const int R = BN_BLOCK / width;
    const int t = threadIdx.x;
    const int c = t % width, rr = t / width;
    if (rr >= R) return;
    const int col = c0 + c;
    const float m = mean[col], s = invstd[col], g = gamma[col];
    float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f;
    if (MODE == 0) {
        k0 = beta[col];
    } else {
        const double N = count[0];
        k0 = g * s;
        k1 = (float)(sums[col] / N);
        k2 = (float)(sums[C + col] / N);
    }
    for (int64_t r = (int64_t)blockIdx.x * R + rr; r < n; r += (int64_t)gridDim.x * R) {
        const int64_t i = r * C + col;
        const float xh = (bn_load(x, i) - m) * s;
        if (MODE == 0) {
            out[i] = (T)(xh * g + k0);
        } else {
            out[i] = (T)(k0 * ((bn_load(dy, i) - k1) - xh * k2));
        }
    }
}

static inline dim3 bn_apply_grid(int64_t n, int C) {
    const int width = C < BN_TILE ? C : BN_TILE;
    const int64_t rows_per_block = (int64_t)(BN_BLOCK / width) * BN_APPLY_ROWS_PER_LANE;
    int64_t bx = st_div_up(n, rows_per_block);
    if (bx > BN_APPLY_MAX_BLOCKS) bx = BN_APPLY_MAX_BLOCKS;
    return dim3((unsigned)bx, (unsigned)st_div_up(C, BN_TILE));
}

extern "C" int64_t st_bn_workspace_bytes(int64_t n, int C) {
    if (n < 0 || C < 1 || C > BN_MAX_C) return -1;
    return bn_chunks(n, C) * 2 * C * (int64_t)sizeof(double) + 256;
}

static int bn_reduce(const void* x, const void* dy, int half, int64_t n, int C, const float* mean, const float* invstd, int mode,
                     double* out, void* ws, int64_t ws_bytes, hipStream_t stream) {
    const int64_t m = 2 * (int64_t)C + (mode == 0 ? 1 : 0);
    if (n == 0) {  // a rank without rows contributes zeros to the all-reduce
        (void)hipMemsetAsync(out, 0, m * sizeof(double), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    ST_REQUIRE(x != nullptr && (mode == 0 || (dy && mean && invstd)), "batchnorm: null input");
    const int64_t need = st_bn_workspace_bytes(n, C);
    if (ws == nullptr || ws_bytes < need) {
        st_set_error("batchnorm: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
        return ST_ERR_WORKSPACE;
    }
    const int64_t rows = bn_rows_per_chunk(n, C);
    const int nchunks = (int)bn_chunks(n, C);
    double* partial = (double*)ws;
    const dim3 grid((unsigned)nchunks, (unsigned)st_div_up(C, BN_TILE));
    if (half) {
        if (mode == 0)
            hipLaunchKernelGGL((k_bn_partial<stbn_h, 0>), grid, dim3(BN_BLOCK), 0, stream, (const stbn_h*)x, (const stbn_h*)nullptr, n, C,
                               mean, invstd, rows, partial);
        else
            hipLaunchKernelGGL((k_bn_partial<stbn_h, 1>), grid, dim3(BN_BLOCK), 0, stream, (const stbn_h*)x, (const stbn_h*)dy, n, C,
                               mean, invstd, rows, partial);
    } else {
        if (mode == 0)
            hipLaunchKernelGGL((k_bn_partial<float, 0>), grid, dim3(BN_BLOCK), 0, stream, (const float*)x, (const float*)nullptr, n, C,
                               mean, invstd, rows, partial);
        else
            hipLaunchKernelGGL((k_bn_partial<float, 1>), grid, dim3(BN_BLOCK), 0, stream, (const float*)x, (const float*)dy, n, C,
                               mean, invstd, rows, partial);
    }
    hipLaunchKernelGGL(k_bn_final, dim3((unsigned)st_div_up(2 * (int64_t)C, BN_BLOCK / 64)), dim3(BN_BLOCK), 0, stream,
                       (const double*)partial, nchunks, C, n, mode, out);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_bn_stats(const void* x, int half, int64_t n, int C, double* out, void* ws, int64_t ws_bytes, void* stream_) {
    ST_REQUIRE(n >= 0 && C >= 1 && C <= BN_MAX_C && out != nullptr, "bn stats: bad arguments (n %lld, C %d)", (long long)n, C);
    return bn_reduce(x, nullptr, half, n, C, nullptr, nullptr, 0, out, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int st_bn_backward_stats(const void* x, const void* dy, int half, int64_t n, int C, const float* mean, const float* invstd,
                                    double* out, void* ws, int64_t ws_bytes, void* stream_) {
    ST_REQUIRE(n >= 0 && C >= 1 && C <= BN_MAX_C && out != nullptr, "bn backward stats: bad arguments (n %lld, C %d)", (long long)n, C);
    return bn_reduce(x, dy, half, n, C, mean, invstd, 1, out, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int st_bn_apply(const void* x, int half, int64_t n, int C, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, void* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n >= 0 && C >= 1 && C <= BN_MAX_C, "bn apply: bad arguments (n %lld, C %d)", (long long)n, C);
    if (n == 0) return ST_OK;
    ST_REQUIRE(x && y && mean && invstd && gamma && beta, "bn apply: null input");
    const dim3 grid = bn_apply_grid(n, C);
    if (half)
        hipLaunchKernelGGL((k_bn_apply<stbn_h, 0>), grid, dim3(BN_BLOCK), 0, stream, (const stbn_h*)x, (const stbn_h*)nullptr, n, C, mean,
                           invstd, gamma, beta, (const double*)nullptr, (const double*)nullptr, (stbn_h*)y);
    else
        hipLaunchKernelGGL((k_bn_apply<float, 0>), grid, dim3(BN_BLOCK), 0, stream, (const float*)x, (const float*)nullptr, n, C, mean,
                           invstd, gamma, beta, (const double*)nullptr, (const double*)nullptr, (float*)y);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_bn_backward_apply(const void* x, const void* dy, int half, int64_t n, int C, const float* mean, const float* invstd,
                                    const float* gamma, const double* sums, const double* count, void* dx, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n >= 0 && C >= 1 && C <= BN_MAX_C, "bn backward apply: bad arguments (n %lld, C %d)", (long long)n, C);
    if (n == 0) return ST_OK;
    ST_REQUIRE(x && dy && dx && mean && invstd && gamma && sums && count, "bn backward apply: null input");
    const dim3 grid = bn_apply_grid(n, C);
    if (half)
        hipLaunchKernelGGL((k_bn_apply<stbn_h, 1>), grid, dim3(BN_BLOCK), 0, stream, (const stbn_h*)x, (const stbn_h*)dy, n, C, mean,
                           invstd, gamma, (const float*)nullptr, sums, count, (stbn_h*)dx);
    else
        hipLaunchKernelGGL((k_bn_apply<float, 1>), grid, dim3(BN_BLOCK), 0, stream, (const float*)x, (const float*)dy, n, C, mean,
                           invstd, gamma, (const float*)nullptr, sums, count, (float*)dx);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
