// st_ground_extent / st_ground_model / st_ground_height: a terrain raster under a cloud, which cells and points are ground, and every
// point's height above it.  A progressive morphological filter (Zhang et al. 2003) on a raster of per-cell minima: every decision is a
// minimum, a maximum, one float32 subtraction or one comparison, so the outputs are the same bits in every run, for a batch and for
// its clouds alone, and equal tests/ground_oracle.py, which restates the header on its own.
//
// The reference has no notion of terrain: its clouds hold trees only.
//
// The contract is in include/smarttree_hip.h.  How it is computed:
// k_gd_extent: the ordered minimum and maximum of the two plan coordinates per cloud.  A thread keeps the extrema of the run of
//   equal clouds it reads (GD_TILES points) in registers, hands each run to a per-workgroup LDS table (one row per cloud) and the
//   workgroup flushes every row that met a point once.  floorf((p - a0) / cell) does not decrease with p (a float32 subtraction and
//   a division by a positive cell round monotonically), so the largest cell index is the index of the largest coordinate:
//   k_gd_dims takes the dimensions from the four extrema.
// k_gd_raster: one atomicMin per point on the ordered bits of its up-coordinate, skipped when the slot already holds a value that
//   is not larger -- a value only decreases, so a stale read costs an atomic that changes nothing, never a missed one.
// k_gd_open: one launch per window.  A workgroup owns a GD_TILE x GD_TILE tile of one cloud's raster and loads it with a halo of
//   2 w cells into LDS (cells outside the raster read +inf).  Four passes in place, one thread per line walking it upwards so
//   that a value is overwritten only after its last reader has passed: minimum along b, minimum along a (the erosion E, set to
//   +inf outside the raster so that the clipped window's maximum does not see it), maximum over finite values along b, then along
//   a (the opening O).  The pitch is odd: the lanes of a pass along b sit on different banks.  A tile reads the previous raster
//   and writes the next one, so no tile sees another's update.
// k_gd_height: one thread per query, four gathers around it.
// Enqueue-only: no allocation, no read-back, no wait.
#include "st_common.h"
#include "st_grid.h"
#include "st_tube.h"

#define GD_BLOCK 256
#define GD_TILES 8         // points per workgroup of the extent pass = GD_TILES * GD_BLOCK, strided by GD_BLOCK
#define GD_TILE 32         // inner cells of a workgroup of the opening, per side
#define GD_MAX_W 32        // largest half-width of a window
#define GD_MAX_K 16
#define GD_REGION (GD_TILE + 4 * GD_MAX_W)  // 160 lines at most
#define GD_PITCH (GD_REGION + 1)            // odd
#define GD_MAX_SIDE 16384
#define GD_MAX_CELLS (1ll << 26)
#define GD_ORD_POS_INF 0xff800000u  // st_f2ord(+inf)
#define GD_ORD_NEG_INF 0x007fffffu  // st_f2ord(-inf)
#define GD_INF __uint_as_float(0x7f800000u)

// The clouds of a call, by value: dimensions, first cell and first tile of each.
struct GdClouds {
    int A[ST_MAX_SEG], B[ST_MAX_SEG];
    long long off[ST_MAX_SEG];
    int tile_off[ST_MAX_SEG + 1];
};

__device__ __forceinline__ void gd_axes(int up, int* a, int* b) {
    *a = up == 0 ? 1 : 0;
    *b = up == 2 ? 1 : 2;
}

// floorf(q) as an index clamped into [0, n - 1], clamped as a float: an overflowed quotient has an index too.  n >= 1.
__device__ __forceinline__ int gd_clamped(float f, int n) { return (int)fminf(fmaxf(f, 0.0f), (float)(n - 1)); }

// ------------------------------------------------------------------------------------------------- extent ---
__global__ void __launch_bounds__(GD_BLOCK) k_gd_extent_init(unsigned* ext, int nseg) {
    const int g = blockIdx.x * GD_BLOCK + threadIdx.x;
    if (g < 4 * nseg) ext[g] = (g & 3) < 2 ? GD_ORD_POS_INF : GD_ORD_NEG_INF;
}

// ext [4 * nseg]: per cloud min a, min b, max a, max b as ordered bits.
__global__ void __launch_bounds__(GD_BLOCK) k_gd_extent(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ seg_off,
                                                        int nseg, int up, unsigned* ext) {
    __shared__ unsigned tab[4 * ST_MAX_SEG];
    for (int j = threadIdx.x; j < 4 * ST_MAX_SEG; j += GD_BLOCK) tab[j] = (j & 3) < 2 ? GD_ORD_POS_INF : GD_ORD_NEG_INF;
    __syncthreads();
    int ax, bx;
    gd_axes(up, &ax, &bx);
    const int64_t base = (int64_t)blockIdx.x * (GD_TILES * GD_BLOCK);
    int run = -1;
    unsigned lo_a = GD_ORD_POS_INF, lo_b = GD_ORD_POS_INF, hi_a = GD_ORD_NEG_INF, hi_b = GD_ORD_NEG_INF;
    for (int tile = 0; tile < GD_TILES; tile++) {
        const int64_t i = base + (int64_t)tile * GD_BLOCK + threadIdx.x;
        if (i >= n) break;
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (!(st_finite(x) && st_finite(y) && st_finite(z))) continue;
        const int s = st_seg_find(seg_off, nseg, i);
        if (s != run) {
            if (run >= 0) {
                atomicMin(&tab[4 * run], lo_a); atomicMin(&tab[4 * run + 1], lo_b);
                atomicMax(&tab[4 * run + 2], hi_a); atomicMax(&tab[4 * run + 3], hi_b);
            }
            run = s;
            lo_a = lo_b = GD_ORD_POS_INF;
            hi_a = hi_b = GD_ORD_NEG_INF;
        }
        const float p[3] = {x, y, z};
        const unsigned oa = st_f2ord(p[ax]), ob = st_f2ord(p[bx]);
        lo_a = st_min(lo_a, oa); hi_a = st_max(hi_a, oa);
        lo_b = st_min(lo_b, ob); hi_b = st_max(hi_b, ob);
    }
    if (run >= 0) {
        atomicMin(&tab[4 * run], lo_a); atomicMin(&tab[4 * run + 1], lo_b);
        atomicMax(&tab[4 * run + 2], hi_a); atomicMax(&tab[4 * run + 3], hi_b);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 4 * nseg; j += GD_BLOCK) {
        const unsigned v = tab[j];
        if ((j & 3) < 2) { if (v != GD_ORD_POS_INF) atomicMin(&ext[j], v); }
        else if (v != GD_ORD_NEG_INF) atomicMax(&ext[j], v);
    }
}

__global__ void __launch_bounds__(GD_BLOCK) k_gd_dims(const unsigned* __restrict__ ext, int nseg, float cell, float* origin, int32_t* dims) {
    const int s = blockIdx.x * GD_BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const bool any = ext[4 * s] != GD_ORD_POS_INF;  // a cloud without a participating point: origin +inf, no cells
    for (int k = 0; k < 2; k++) {
        const float lo = st_ord2f(ext[4 * s + k]), hi = st_ord2f(ext[4 * s + 2 + k]);
        origin[2 * s + k] = lo;
        dims[2 * s + k] = any ? (int)fminf(fmaxf(floorf((hi - lo) / cell), 0.0f), 1073741824.0f - 1.0f) + 1 : 0;
    }
}

// -------------------------------------------------------------------------------------------------- model ---
__global__ void __launch_bounds__(GD_BLOCK) k_gd_fill(unsigned* zord, int64_t cells) {
    const int64_t c = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (c < cells) zord[c] = GD_ORD_POS_INF;
}

__global__ void __launch_bounds__(GD_BLOCK) k_gd_raster(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ seg_off,
                                                        int nseg, int up, float cell, const float* __restrict__ origin, GdClouds C,
                                                        unsigned* zord) {
    const int64_t i = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (!(st_finite(p[0]) && st_finite(p[1]) && st_finite(p[2]))) return;
    int ax, bx;
    gd_axes(up, &ax, &bx);
    const int s = st_seg_find(seg_off, nseg, i);
    const float fa = floorf((p[ax] - origin[2 * s]) / cell), fb = floorf((p[bx] - origin[2 * s + 1]) / cell);
    // with the extent's own origin and dimensions every participating point is inside; one that is not takes no part
    if (!(fa >= 0.0f && fa < (float)C.A[s] && fb >= 0.0f && fb < (float)C.B[s])) return;
    unsigned* slot = zord + C.off[s] + (long long)(int)fa * C.B[s] + (int)fb;
    const unsigned o = st_f2ord(p[up]);
    if (*slot > o) atomicMin(slot, o);
}

__global__ void __launch_bounds__(GD_BLOCK) k_gd_unpack(const unsigned* __restrict__ zord, int64_t cells, float* z, uint8_t* flags) {
    const int64_t c = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const unsigned o = zord[c];
    z[c] = st_ord2f(o);
    flags[c] = o == GD_ORD_POS_INF ? 1 : 0;
}

// One window of half-width w and threshold dh: zout = the opening of zin where zin stands more than dh above it, else zin.
__global__ void __launch_bounds__(GD_BLOCK) k_gd_open(const float* __restrict__ zin, float* __restrict__ zout, uint8_t* flags, int w,
                                                      float dh, GdClouds C, int nseg) {
    __shared__ unsigned s[GD_REGION * GD_PITCH];  // ordered bits: integer minima and maxima, -0 below +0 as in the raster
    int c = 0;  // the cloud of this tile (tile_off is ascending; a cloud without cells has no tile)
    {
        int lo = 0, hi = nseg;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (C.tile_off[mid] <= (int)blockIdx.x) lo = mid; else hi = mid; }
        c = lo;
    }
    const int A = C.A[c], B = C.B[c];
    const int tiles_b = (B + GD_TILE - 1) / GD_TILE, t = (int)blockIdx.x - C.tile_off[c];
    const int a_in = (t / tiles_b) * GD_TILE, b_in = (t % tiles_b) * GD_TILE;  // the first inner cell
    const int R = GD_TILE + 4 * w, R1 = GD_TILE + 2 * w, win = 2 * w + 1;
    const float* zc = zin + C.off[c];
    // region cell (r, q) is raster cell (a_in - 2w + r, b_in - 2w + q)
    for (int j = threadIdx.x; j < R * R; j += GD_BLOCK) {
        const int r = j / R, q = j - r * R, ga = a_in - 2 * w + r, gb = b_in - 2 * w + q;
        s[r * GD_PITCH + q] = (ga >= 0 && ga < A && gb >= 0 && gb < B) ? st_f2ord(zc[(long long)ga * B + gb]) : GD_ORD_POS_INF;
    }
    __syncthreads();
    // minimum along b: s[r][q] <- min s[r][q .. q + 2w], the value of region column q + w
    for (int r = threadIdx.x; r < R; r += GD_BLOCK) {
        unsigned* line = s + r * GD_PITCH;
        for (int q = 0; q < R1; q++) {
            unsigned m = line[q];
#pragma unroll 8
            for (int d = 1; d < win; d++) m = st_min(m, line[q + d]);
            line[q] = m;
        }
    }
    __syncthreads();
    // minimum along a: s[r][q] <- E of region cell (r + w, q + w); +inf where that cell is outside the raster
    for (int q = threadIdx.x; q < R1; q += GD_BLOCK) {
        const int gb = b_in - w + q;
        for (int r = 0; r < R1; r++) {
            unsigned m = s[r * GD_PITCH + q];
#pragma unroll 8
            for (int d = 1; d < win; d++) m = st_min(m, s[(r + d) * GD_PITCH + q]);
            const int ga = a_in - w + r;
            s[r * GD_PITCH + q] = (ga >= 0 && ga < A && gb >= 0 && gb < B) ? m : GD_ORD_POS_INF;
        }
    }
    __syncthreads();
    // maximum over finite values along b: 0 (below the bits of every float) stands for "none"
    for (int r = threadIdx.x; r < R1; r += GD_BLOCK) {
        unsigned* line = s + r * GD_PITCH;
        for (int q = 0; q < GD_TILE; q++) {
            unsigned m = 0u;
#pragma unroll 8
            for (int d = 0; d < win; d++) { const unsigned v = line[q + d]; if (v < GD_ORD_POS_INF) m = st_max(m, v); }
            line[q] = m;
        }
    }
    __syncthreads();
    // maximum along a, the decision and the write
    for (int q = threadIdx.x; q < GD_TILE; q += GD_BLOCK) {
        const int gb = b_in + q;
        if (gb >= B) continue;
        for (int r = 0; r < GD_TILE; r++) {
            const int ga = a_in + r;
            if (ga >= A) break;
            unsigned m = 0u;
#pragma unroll 8
            for (int d = 0; d < win; d++) m = st_max(m, s[(r + d) * GD_PITCH + q]);
            const float o = m == 0u ? GD_INF : st_ord2f(m);
            const long long cellx = C.off[c] + (long long)ga * B + gb;
            float z = zin[cellx];
            if (z - o > dh) {
                flags[cellx] |= 2;
                z = o;
            }
            zout[cellx] = z;
        }
    }
}

// ------------------------------------------------------------------------------------------------- height ---
__global__ void __launch_bounds__(GD_BLOCK) k_gd_height(const float* __restrict__ pts, int64_t m, const int32_t* __restrict__ seg_off,
                                                        int nseg, int up, float cell, float tol, const float* __restrict__ origin,
                                                        GdClouds C, const float* __restrict__ surface, float* height, uint8_t* is_ground,
                                                        float* ground) {
    const int64_t i = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (i >= m) return;
    const float nan = __uint_as_float(0x7fc00000u);
    float h = nan, g = nan;
    uint8_t is = 0;
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const int c = st_seg_find(seg_off, nseg, i);
    const int A = C.A[c], B = C.B[c];
    if (st_finite(p[0]) && st_finite(p[1]) && st_finite(p[2]) && A > 0 && B > 0) {
        int ax, bx;
        gd_axes(up, &ax, &bx);
        const float* sf = surface + C.off[c];
        const float qa = (p[ax] - origin[2 * c]) / cell, qb = (p[bx] - origin[2 * c + 1]) / cell;
        const float own = sf[(long long)gd_clamped(floorf(qa), A) * B + gd_clamped(floorf(qb), B)];
        if (st_finite(own)) {
            is = (p[up] - own <= tol) ? 1 : 0;
            const float fa = qa - 0.5f, fb = qb - 0.5f;
            const float a0 = floorf(fa), b0 = floorf(fb);
            const float ta = fa - a0, tb = fb - b0;
            const long long i0 = gd_clamped(a0, A), i1 = gd_clamped(a0 + 1.0f, A);
            const int j0 = gd_clamped(b0, B), j1 = gd_clamped(b0 + 1.0f, B);
            float s00 = sf[i0 * B + j0], s01 = sf[i0 * B + j1], s10 = sf[i1 * B + j0], s11 = sf[i1 * B + j1];
            if (!st_finite(s00)) s00 = own;
            if (!st_finite(s01)) s01 = own;
            if (!st_finite(s10)) s10 = own;
            if (!st_finite(s11)) s11 = own;
            const float s0 = s00 + tb * (s01 - s00), s1 = s10 + tb * (s11 - s10);
            g = s0 + ta * (s1 - s0);
            h = p[up] - g;
        }
    }
    if (height) height[i] = h;
    if (is_ground) is_ground[i] = is;
    if (ground) ground[i] = g;
}

// --------------------------------------------------------------------------------------------------- host ---
struct GdLayout {
    unsigned* ext;
    unsigned* zord;
    float* z0;
    float* z1;
};

static void gd_layout(StArena& a, int64_t cells, GdLayout* L) {
    L->ext = a.take<unsigned>(4 * ST_MAX_SEG);
    L->zord = a.take<unsigned>(cells);
    L->z0 = a.take<float>(cells);
    L->z1 = a.take<float>(cells);
}

extern "C" int64_t st_ground_workspace_bytes(int64_t cells) {
    if (cells < 0 || cells > GD_MAX_CELLS) return -1;
    StArena a(nullptr, 0);
    GdLayout L;
    gd_layout(a, cells, &L);
    return a.used;
}

// The clouds' table from the host arrays; false (error text set, starting with `who`) when they do not fit together.
static bool gd_clouds(const char* who, const int32_t* dims, const int64_t* cell_off, int nseg, GdClouds* C, int64_t* cells) {
    if (!dims || !cell_off) {
        st_set_error("%s: the dimensions and the cell offsets are host arrays and may not be NULL", who);
        return false;
    }
    memset(C, 0, sizeof(*C));
    int64_t at = 0, tiles = 0;
    for (int s = 0; s < nseg; s++) {
        const int64_t A = dims[2 * s], B = dims[2 * s + 1];
        if (A < 0 || B < 0 || A > GD_MAX_SIDE || B > GD_MAX_SIDE || (A == 0) != (B == 0)) {
            st_set_error("%s: cloud %d has %lld x %lld cells; a side is 0..%d, both or neither 0 (choose a larger cell)", who, s, (long long)A,
                         (long long)B, GD_MAX_SIDE);
            return false;
        }
        if (cell_off[s] != at) {
            st_set_error("%s: cell_off[%d] = %lld does not follow from the dimensions (%lld)", who, s, (long long)cell_off[s], (long long)at);
            return false;
        }
        C->A[s] = (int)A;
        C->B[s] = (int)B;
        C->off[s] = at;
        C->tile_off[s] = (int)tiles;
        at += A * B;
        tiles += st_div_up(A, GD_TILE) * st_div_up(B, GD_TILE);
        if (at > GD_MAX_CELLS) {
            st_set_error("%s: more than 2^26 cells in one call (choose a larger cell)", who);
            return false;
        }
    }
    if (cell_off[nseg] != at) {
        st_set_error("%s: cell_off[%d] = %lld does not follow from the dimensions (%lld)", who, nseg, (long long)cell_off[nseg], (long long)at);
        return false;
    }
    C->tile_off[nseg] = (int)tiles;
    *cells = at;
    return true;
}

#define GD_COMMON(who, count)                                                                                                    \
    ST_REQUIRE(count >= 0 && count < (1ll << 31), who ": 0 <= points < 2^31 (got %lld)", (long long)count);                       \
    ST_REQUIRE(nseg >= 1 && nseg <= ST_MAX_SEG, who ": 1 <= clouds per batch <= %d (got %d)", ST_MAX_SEG, nseg);                   \
    ST_REQUIRE(nseg == 1 || seg_off, who ": %d clouds need the offsets of their points", nseg);                                    \
    ST_REQUIRE(up >= 0 && up <= 2, who ": the vertical axis is 0, 1 or 2 (got %d)", up);                                           \
    ST_REQUIRE(cell > 0.0f && cell <= 3.4028234e38f, who ": the cell size must be finite and > 0 (got %g)", (double)cell)

extern "C" int st_ground_extent(const float* pts, int64_t n, const int32_t* seg_off, int nseg, int up, float cell, float* origin,
                                int32_t* dims, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GD_COMMON("ground_extent", n);
    ST_REQUIRE(n == 0 || pts, "ground_extent: %lld points need their coordinates", (long long)n);
    ST_REQUIRE(origin && dims, "ground_extent: the origin and the dimensions may not be NULL");
    StArena arena(ws, ws_bytes);
    GdLayout L;
    gd_layout(arena, 0, &L);
    if (!arena.ok() || !ws) {
        st_set_error("ground_extent: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (nseg == 1) seg_off = nullptr;
    hipLaunchKernelGGL(k_gd_extent_init, dim3(1), dim3(GD_BLOCK), 0, stream, L.ext, nseg);
    if (n > 0)
        hipLaunchKernelGGL(k_gd_extent, dim3((unsigned)st_div_up(n, GD_TILES * GD_BLOCK)), dim3(GD_BLOCK), 0, stream, pts, n, seg_off, nseg, up,
                           L.ext);
    hipLaunchKernelGGL(k_gd_dims, dim3(1), dim3(GD_BLOCK), 0, stream, (const unsigned*)L.ext, nseg, cell, origin, dims);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_ground_model(const float* pts, int64_t n, const int32_t* seg_off, int nseg, int up, float cell, const float* origin,
                               const int32_t* dims_host, const int64_t* cell_off_host, int n_windows, const int32_t* w_host,
                               const float* dh_host, float* surface, uint8_t* flags, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GD_COMMON("ground_model", n);
    ST_REQUIRE(n_windows >= 1 && n_windows <= GD_MAX_K, "ground_model: 1 <= windows <= %d (got %d)", GD_MAX_K, n_windows);
    ST_REQUIRE(w_host && dh_host, "ground_model: the windows and their thresholds are host arrays and may not be NULL");
    for (int k = 0; k < n_windows; k++) {
        ST_REQUIRE(w_host[k] >= 1 && w_host[k] <= GD_MAX_W && (k == 0 || w_host[k] > w_host[k - 1]),
                   "ground_model: window half-widths are 1..%d cells and strictly increasing (window %d is %d)", GD_MAX_W, k, w_host[k]);
        ST_REQUIRE(dh_host[k] == dh_host[k], "ground_model: the threshold of window %d is NaN", k);
    }
    ST_REQUIRE(n == 0 || pts, "ground_model: %lld points need their coordinates", (long long)n);
    GdClouds C;
    int64_t cells = 0;
    if (!gd_clouds("ground_model", dims_host, cell_off_host, nseg, &C, &cells)) return ST_ERR_INVALID;
    ST_REQUIRE(origin, "ground_model: the origin may not be NULL");
    ST_REQUIRE(cells == 0 || (surface && flags), "ground_model: %lld cells need their surface and flags", (long long)cells);
    StArena arena(ws, ws_bytes);
    GdLayout L;
    gd_layout(arena, cells, &L);
    if (!arena.ok() || !ws) {
        st_set_error("ground_model: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (cells == 0) return ST_OK;
    if (nseg == 1) seg_off = nullptr;
    const unsigned cb = (unsigned)st_div_up(cells, GD_BLOCK);
    hipLaunchKernelGGL(k_gd_fill, dim3(cb), dim3(GD_BLOCK), 0, stream, L.zord, cells);
    if (n > 0)
        hipLaunchKernelGGL(k_gd_raster, dim3((unsigned)st_div_up(n, GD_BLOCK)), dim3(GD_BLOCK), 0, stream, pts, n, seg_off, nseg, up, cell,
                           origin, C, L.zord);
    hipLaunchKernelGGL(k_gd_unpack, dim3(cb), dim3(GD_BLOCK), 0, stream, (const unsigned*)L.zord, cells, L.z0, flags);
    const float* cur = L.z0;
    for (int k = 0; k < n_windows; k++) {
        float* dst = k == n_windows - 1 ? surface : (cur == L.z0 ? L.z1 : L.z0);
        hipLaunchKernelGGL(k_gd_open, dim3((unsigned)C.tile_off[nseg]), dim3(GD_BLOCK), 0, stream, cur, dst, flags, (int)w_host[k], dh_host[k],
                           C, nseg);
        cur = dst;
    }
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_ground_height(const float* pts, int64_t m, const int32_t* seg_off, int nseg, int up, float cell, float tol,
                                const float* origin, const int32_t* dims_host, const int64_t* cell_off_host, const float* surface,
                                float* height, uint8_t* is_ground, float* ground, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GD_COMMON("ground_height", m);
    ST_REQUIRE(tol == tol, "ground_height: the tolerance is NaN");
    ST_REQUIRE(m == 0 || pts, "ground_height: %lld points need their coordinates", (long long)m);
    GdClouds C;
    int64_t cells = 0;
    if (!gd_clouds("ground_height", dims_host, cell_off_host, nseg, &C, &cells)) return ST_ERR_INVALID;
    ST_REQUIRE(origin, "ground_height: the origin may not be NULL");
    ST_REQUIRE(cells == 0 || surface, "ground_height: %lld cells need their surface", (long long)cells);
    if (m == 0) return ST_OK;
    if (nseg == 1) seg_off = nullptr;
    hipLaunchKernelGGL(k_gd_height, dim3((unsigned)st_div_up(m, GD_BLOCK)), dim3(GD_BLOCK), 0, stream, pts, m, seg_off, nseg, up, cell, tol,
                       origin, C, surface, height, is_ground, ground);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
