// st_render_*: an offscreen software rasteriser for labelled clouds and skeletons -- points (pixels or discs), screen-space capsules
// (skeleton tubes, and 1-pixel lines for the medial vectors), and a resolve pass that turns the framebuffer into images.
//
// Replaces  o3d_abstractions/camera.py:71-101 (Renderer.capture through open3d's OffscreenRenderer) and the to_o3d_* geometry
//           the reference builds on the host for it (model/render.py:7-35).  Here the device tensors the pipeline already holds are
//           drawn where they are; nothing is copied to the host to be drawn.
//
// Framebuffer.  fb [V,H,W] unsigned long long in the caller's workspace, cleared to all ones = background.  A covered pixel is
// offered key = (bits of the float32 depth) << 32 | id with ONE atomicMin: depths are positive (z > near > 0), so their bit patterns
// order as the floats do, the smallest depth wins and equal depths go to the lowest id.  A minimum does not depend on the order of
// arrival: the images are bit-identical from run to run.  Ids are id_base + index; the caller hands every item of a frame its own
// range (points of item 0, then item 1's, ...).  Before the atomic the lane reads fb[pix] with a plain load and skips the atomic
// when its key is not smaller (as st_hash_insert_min_dup, st_common.h): a value only decreases, so a stale read can cost a needless
// atomic and never skips a needed one -- a hidden point costs a load that hits in L2 instead of an 8-byte atomic that drops the line.
//
// Cameras.  cams [V,16] float32 (device): R row-major (9), t (3), fx, fy, cx, cy.  A pixel (column u, row v) has its centre AT the
// integer (u, v).  All arithmetic is float32 in exactly the order below, contraction off (tests/render_oracle.py restates it):
//   camera space   xc = ((R00*px + R01*py) + R02*pz) + tx, yc and zc likewise with rows 1 and 2
//   culled         !(zc > near), or xc / yc / zc not finite
//   projection     u = (fx*xc)/zc + cx,  v = (fy*yc)/zc + cy;  culled when u or v is not finite
//
// Points.  rp = max(point_px/2, (fx*r)/zc) (r: the optional world radius; a NaN r counts as none).  The point always goes to its
// nearest pixel (floor(u + 0.5), floor(v + 0.5)); with rp > 0.5 it also covers every pixel centre (i, j) of
// [ceil(u-rp), floor(u+rp)] x [ceil(v-rp), floor(v+rp)] with (i-u)^2 + (j-v)^2 <= rp*rp (a radius whose square leaves float32 draws
// no disc).  Depth zc.  point_px = 1: one pixel.
//
// Segments (a, b, r1, r2).  Ends in camera space as above; a non-finite end or radius culls the segment, both ends at z <= near too.
// An end at z <= near is moved to the near plane: t = (near - z)/(z' - z) (z' the other end's), x += t*(x' - x), y likewise,
// r += t*(r' - r), z = near.  Ends project to (ua, va), (ub, vb) with pixel radii pa = max((fx*ra)/za, min_px/2), pb likewise; a
// non-finite projection or radius culls.  For the pixel centre q = (i, j):
//   e = b' - a', L2 = ex*ex + ey*ey, s = L2 > 0 ? clamp(((i-ua)*ex + (j-va)*ey)/L2, 0, 1) : 0
//   dx = i - (ua + s*ex), dy = j - (va + s*ey), d = sqrtf(dx*dx + dy*dy), rp = pa + s*(pb - pa);  covered iff d <= rp
//   zx = 1/((1-s)/za + s/zb), k = rp > 0 ? d/rp : 0, depth = max(near, zx*(1 - (rp/fx)*sqrtf(max(0, 1 - k*k))))
// i.e. the front of a sphere of the interpolated radius around the perspective-correct axis point (an impostor; a capsule that
// encloses the eye is cut at the near plane).  The pixels walked are [ceil(min(ua-pa, ub-pb)), floor(max(ua+pa, ub+pb))] x (rows
// likewise), clipped to the viewport BEFORE any loop or conversion to int: every covered pixel lies in the hull of the two end discs.
//
// Work distribution of the segments.  1M medial-vector lines of a few pixels and 10k capsules up to hundreds of pixels wide go
// through the same two launches.  k_rs_segments_small: one LANE per segment, all V views; a (segment, view) whose clipped box is at
// most RS_SMALL_AREA pixels is drawn there, a larger one is appended to a queue in the workspace.  k_rs_segments_large: a fixed
// grid, one WAVEFRONT per queue entry (grid-stride), the lanes striding over the box.  The queue has RS_QUEUE entries; one that does
// not fit is drawn by the lane that found it (slow, correct).  The queue's order varies from run to run, the framebuffer does not.
//
// Resolve.  One lane per pixel: depth (+inf on the background), id (-1) and colour.  The colour is looked up per visible PIXEL
// (H*W gathers, not N) in the item that owns the id: 0 uniform | 1 float rgb [n,3] | 2 class int32 [n] through cmap [C,3] (outside
// [0,C): black) | 3 scalar float [n] through the ramp t = clamp((x-lo)/(hi-lo), 0, 1) (NaN -> 0), x4 = t*4, k = min((int)x4, 3),
// c = stop[k] + (x4-k)*(stop[k+1]-stop[k]) over blue, cyan, green, yellow, red | 4 int32 id [n] through a hash (bytes of
// st_hash64(id + 1), each halved and lifted by 64: neither near white nor near black).  Eye-dome shading (edl_strength > 0), from
// the depths alone: shade = expf(-strength * sum over the neighbours (x-e, x+e, y-e, y+e in this order, inside the image, not
// background) of max(0, log2f(z) - log2f(z_nb))).  byte = floorf(clamp(c*shade, 0, 1)*255 + 0.5) (c alone without shading).
// Background pixels are white.
#include "st_common.h"
#include "smarttree_hip.h"  // StRenderItem, and the declarations of the entry points below

#define RS_BLOCK 256
#define RS_SMALL_AREA 64         // pixels of a clipped box one lane still walks itself
#define RS_QUEUE (1ll << 18)      // (segment, view) entries of the large-segment queue
#define RS_LARGE_BLOCKS 2048      // grid of k_rs_segments_large: 8192 wavefronts = 8 per SIMD of 256 CUs
#define RS_MAX_ITEMS 16
#define RS_MAX_DIM 16384
#define RS_FLT_MAX 3.402823466e+38f
#define RS_BG 0xffffffffffffffffull

struct RsItems {
    int n;
    int32_t id_end[RS_MAX_ITEMS];
    int32_t mode[RS_MAX_ITEMS], n_classes[RS_MAX_ITEMS];
    const void* data[RS_MAX_ITEMS];
    const float* cmap[RS_MAX_ITEMS];
    float lo[RS_MAX_ITEMS], hi[RS_MAX_ITEMS], rgb[RS_MAX_ITEMS][3];
};

struct RsCam {
    float r[9], t[3], fx, fy, cx, cy;
};

__device__ __forceinline__ bool rs_finite(float v) { return fabsf(v) <= RS_FLT_MAX; }  // false for NaN

__device__ __forceinline__ RsCam rs_load_cam(const float* __restrict__ cams, int v) {
    RsCam c;
    const float* p = cams + 16 * (int64_t)v;
#pragma unroll
    for (int k = 0; k < 9; k++) c.r[k] = p[k];
    c.t[0] = p[9]; c.t[1] = p[10]; c.t[2] = p[11];
    c.fx = p[12]; c.fy = p[13]; c.cx = p[14]; c.cy = p[15];
    return c;
}

__device__ __forceinline__ void rs_to_camera(const RsCam& c, float px, float py, float pz, float& x, float& y, float& z) {
    x = ((c.r[0] * px + c.r[1] * py) + c.r[2] * pz) + c.t[0];
    y = ((c.r[3] * px + c.r[4] * py) + c.r[5] * pz) + c.t[1];
    z = ((c.r[6] * px + c.r[7] * py) + c.r[8] * pz) + c.t[2];
}

__device__ __forceinline__ void rs_offer(unsigned long long* __restrict__ fb, int64_t pix, float depth, unsigned id) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)id;
    if (key < fb[pix]) atomicMin(&fb[pix], key);
}

// ---- points ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RS_BLOCK) k_rs_points(const float* __restrict__ xyz, const float* __restrict__ radius, int64_t n,
                                                        unsigned id_base, float point_px, const float* __restrict__ cams, int V, int H,
                                                        int W, float near, unsigned long long* __restrict__ fb) {
    const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const float r = radius ? radius[i] : 0.0f;
    const unsigned id = id_base + (unsigned)i;
    const float half_px = point_px * 0.5f;
    for (int v = 0; v < V; v++) {
        const RsCam c = rs_load_cam(cams, v);
        float xc, yc, zc;
        rs_to_camera(c, px, py, pz, xc, yc, zc);
        if (!(zc > near) || !rs_finite(xc) || !rs_finite(yc) || !rs_finite(zc)) continue;
        const float u = (c.fx * xc) / zc + c.cx, w = (c.fy * yc) / zc + c.cy;
        if (!rs_finite(u) || !rs_finite(w)) continue;
        unsigned long long* img = fb + (int64_t)v * H * W;
        const float rp = radius ? fmaxf(half_px, (c.fx * r) / zc) : half_px;
        const float fu = floorf(u + 0.5f), fw = floorf(w + 0.5f);
        const bool inside = fu >= 0.0f && fu < (float)W && fw >= 0.0f && fw < (float)H;
        const int iu = inside ? (int)fu : -1, iw = inside ? (int)fw : -1;
        if (inside) rs_offer(img, (int64_t)iw * W + iu, zc, id);
        const float rp2 = rp * rp;
        if (!(rp > 0.5f) || !rs_finite(rp2)) continue;  // with rp2 = inf an overflowing dx*dx would pass the disc test
        const float x0f = fmaxf(ceilf(u - rp), 0.0f), x1f = fminf(floorf(u + rp), (float)(W - 1));
        const float y0f = fmaxf(ceilf(w - rp), 0.0f), y1f = fminf(floorf(w + rp), (float)(H - 1));
        if (!(x0f <= x1f && y0f <= y1f)) continue;
        const int x0 = (int)x0f, x1 = (int)x1f, y0 = (int)y0f, y1 = (int)y1f;
        for (int y = y0; y <= y1; y++) {
            const float dy = (float)y - w;
            for (int x = x0; x <= x1; x++) {
                const float dx = (float)x - u;
                if (dx * dx + dy * dy <= rp2 && !(x == iu && y == iw)) rs_offer(img, (int64_t)y * W + x, zc, id);
            }
        }
    }
}

// ---- segments ----------------------------------------------------------------------------------------------------------
struct RsSeg {
    float ua, va, ub, vb, pa, pb, za, zb, fx;
    int x0, x1, y0, y1;  // clipped to the viewport; valid only when ok
    bool ok;
};

__device__ __forceinline__ RsSeg rs_segment_setup(const RsCam& c, const float* __restrict__ a, const float* __restrict__ b, float ra,
                                                  float rb, float min_px, float near, int H, int W) {
    RsSeg s;
    s.ok = false;
    s.fx = c.fx;
    float xa, ya, za, xb, yb, zb;
    rs_to_camera(c, a[0], a[1], a[2], xa, ya, za);
    rs_to_camera(c, b[0], b[1], b[2], xb, yb, zb);
    if (!(rs_finite(xa) && rs_finite(ya) && rs_finite(za) && rs_finite(xb) && rs_finite(yb) && rs_finite(zb) && rs_finite(ra) &&
          rs_finite(rb)))
        return s;
    const bool a_in = za > near, b_in = zb > near;
    if (!a_in && !b_in) return s;
    if (!a_in) {
        const float t = (near - za) / (zb - za);
        xa = xa + t * (xb - xa); ya = ya + t * (yb - ya); ra = ra + t * (rb - ra); za = near;
    } else if (!b_in) {
        const float t = (near - zb) / (za - zb);
        xb = xb + t * (xa - xb); yb = yb + t * (ya - yb); rb = rb + t * (ra - rb); zb = near;
    }
    const float half_px = min_px * 0.5f;
    s.ua = (c.fx * xa) / za + c.cx; s.va = (c.fy * ya) / za + c.cy;
    s.ub = (c.fx * xb) / zb + c.cx; s.vb = (c.fy * yb) / zb + c.cy;
    s.pa = fmaxf((c.fx * ra) / za, half_px); s.pb = fmaxf((c.fx * rb) / zb, half_px);
    s.za = za; s.zb = zb;
    if (!(rs_finite(s.ua) && rs_finite(s.va) && rs_finite(s.ub) && rs_finite(s.vb) && rs_finite(s.pa) && rs_finite(s.pb))) return s;
    const float x0f = fmaxf(ceilf(fminf(s.ua - s.pa, s.ub - s.pb)), 0.0f), x1f = fminf(floorf(fmaxf(s.ua + s.pa, s.ub + s.pb)), (float)(W - 1));
    const float y0f = fmaxf(ceilf(fminf(s.va - s.pa, s.vb - s.pb)), 0.0f), y1f = fminf(floorf(fmaxf(s.va + s.pa, s.vb + s.pb)), (float)(H - 1));
    if (!(x0f <= x1f && y0f <= y1f)) return s;
    s.x0 = (int)x0f; s.x1 = (int)x1f; s.y0 = (int)y0f; s.y1 = (int)y1f;
    s.ok = true;
    return s;
}

// (x, y) is inside the viewport: the callers only walk the clipped box
__device__ __forceinline__ void rs_segment_pixel(const RsSeg& g, int x, int y, float near, int W, unsigned long long* __restrict__ img,
                                                 unsigned id) {
    const float qx = (float)x, qy = (float)y;
    const float ex = g.ub - g.ua, ey = g.vb - g.va;
    const float l2 = ex * ex + ey * ey;
    float s = 0.0f;
    if (l2 > 0.0f) {
        s = ((qx - g.ua) * ex + (qy - g.va) * ey) / l2;
        s = s > 0.0f ? (s < 1.0f ? s : 1.0f) : 0.0f;  // a NaN goes to 0
    }
    const float dx = qx - (g.ua + s * ex), dy = qy - (g.va + s * ey);
    const float d = sqrtf(dx * dx + dy * dy);
    const float rp = g.pa + s * (g.pb - g.pa);
    if (!(d <= rp)) return;
    const float zx = 1.0f / ((1.0f - s) / g.za + s / g.zb);
    const float k = rp > 0.0f ? d / rp : 0.0f;
    const float depth = fmaxf(near, zx * (1.0f - (rp / g.fx) * sqrtf(fmaxf(0.0f, 1.0f - k * k))));
    if (!(depth <= RS_FLT_MAX)) return;
    rs_offer(img, (int64_t)y * W + x, depth, id);
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_segments_small(const float* __restrict__ a, const float* __restrict__ b,
                                                                const float* __restrict__ r1, const float* __restrict__ r2, int64_t m,
                                                                unsigned id_base, float min_px, const float* __restrict__ cams, int V,
                                                                int H, int W, float near, unsigned long long* __restrict__ fb,
                                                                unsigned* __restrict__ q_count, unsigned long long* __restrict__ queue) {
    const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= m) return;
    float pa[3], pb[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { pa[k] = a[3 * i + k]; pb[k] = b[3 * i + k]; }
    const float ra = r1[i], rb = r2[i];
    for (int v = 0; v < V; v++) {
        const RsCam c = rs_load_cam(cams, v);
        const RsSeg g = rs_segment_setup(c, pa, pb, ra, rb, min_px, near, H, W);
        if (!g.ok) continue;
        const int64_t area = (int64_t)(g.x1 - g.x0 + 1) * (g.y1 - g.y0 + 1);
        if (area > RS_SMALL_AREA) {
            const unsigned at = atomicAdd(q_count, 1u);
            if (at < (unsigned)RS_QUEUE) {
                queue[at] = ((unsigned long long)i << 16) | (unsigned long long)v;
                continue;
            }
        }
        unsigned long long* img = fb + (int64_t)v * H * W;
        for (int y = g.y0; y <= g.y1; y++)
            for (int x = g.x0; x <= g.x1; x++) rs_segment_pixel(g, x, y, near, W, img, id_base + (unsigned)i);
    }
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_segments_large(const float* __restrict__ a, const float* __restrict__ b,
                                                                const float* __restrict__ r1, const float* __restrict__ r2,
                                                                unsigned id_base, float min_px, const float* __restrict__ cams, int H,
                                                                int W, float near, unsigned long long* __restrict__ fb,
                                                                const unsigned* __restrict__ q_count,
                                                                const unsigned long long* __restrict__ queue) {
    const unsigned lane = threadIdx.x & 63u;
    const int64_t wave = (int64_t)blockIdx.x * (RS_BLOCK / 64) + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * (RS_BLOCK / 64);
    const unsigned filled = *q_count;
    const int64_t count = filled < (unsigned)RS_QUEUE ? (int64_t)filled : RS_QUEUE;
    for (int64_t e = wave; e < count; e += n_waves) {
        const unsigned long long entry = queue[e];
        const int64_t i = (int64_t)(entry >> 16);
        const int v = (int)(entry & 0xffffull);
        const RsCam c = rs_load_cam(cams, v);
        const RsSeg g = rs_segment_setup(c, a + 3 * i, b + 3 * i, r1[i], r2[i], min_px, near, H, W);  // the same box as in the small pass
        if (!g.ok) continue;
        unsigned long long* img = fb + (int64_t)v * H * W;
        const int bw = g.x1 - g.x0 + 1;
        const int64_t area = (int64_t)bw * (g.y1 - g.y0 + 1);
        for (int64_t p = lane; p < area; p += 64) {
            const int y = g.y0 + (int)(p / bw), x = g.x0 + (int)(p % bw);
            rs_segment_pixel(g, x, y, near, W, img, id_base + (unsigned)i);
        }
    }
}

// ---- resolve -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char rs_to8(float c) {
    c = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;  // a NaN goes to 0
    return (unsigned char)(int)floorf(c * 255.0f + 0.5f);
}

__device__ __forceinline__ void rs_colour(const RsItems& I, unsigned id, float& r, float& g, float& b) {
    int it = 0;
    while (it < I.n - 1 && (int32_t)id >= I.id_end[it]) it++;
    const int64_t k = (int64_t)id - (it > 0 ? I.id_end[it - 1] : 0);
    if ((int32_t)id >= I.id_end[it]) {  // an id no item of the table owns (drawn with another table): black, and no gather
        r = g = b = 0.0f;
        return;
    }
    r = I.rgb[it][0]; g = I.rgb[it][1]; b = I.rgb[it][2];
    switch (I.mode[it]) {
    case 1: {
        const float* p = (const float*)I.data[it] + 3 * k;
        r = p[0]; g = p[1]; b = p[2];
        break;
    }
    case 2: {
        const int cl = ((const int32_t*)I.data[it])[k];
        if (cl >= 0 && cl < I.n_classes[it]) {
            const float* p = I.cmap[it] + 3 * (int64_t)cl;
            r = p[0]; g = p[1]; b = p[2];
        } else {
            r = g = b = 0.0f;
        }
        break;
    }
    case 3: {
        const float stop[5][3] = {{0.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 1.0f}, {0.0f, 1.0f, 0.0f}, {1.0f, 1.0f, 0.0f}, {1.0f, 0.0f, 0.0f}};
        float t = (((const float*)I.data[it])[k] - I.lo[it]) / (I.hi[it] - I.lo[it]);
        t = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
        const float x4 = t * 4.0f;
        int s = (int)x4;
        s = s < 3 ? s : 3;
        const float f = x4 - (float)s;
        r = stop[s][0] + f * (stop[s + 1][0] - stop[s][0]);
        g = stop[s][1] + f * (stop[s + 1][1] - stop[s][1]);
        b = stop[s][2] + f * (stop[s + 1][2] - stop[s][2]);
        break;
    }
    case 4: {
        const unsigned long long h = st_hash64((unsigned long long)(long long)((const int32_t*)I.data[it])[k] + 1ull);
        r = (float)(64u + ((unsigned)(h >> 8) & 127u)) / 255.0f;
        g = (float)(64u + ((unsigned)(h >> 24) & 127u)) / 255.0f;
        b = (float)(64u + ((unsigned)(h >> 40) & 127u)) / 255.0f;
        break;
    }
    default: break;
    }
}

__global__ void __launch_bounds__(RS_BLOCK) k_rs_resolve(const unsigned long long* __restrict__ fb, int V, int H, int W, RsItems I,
                                                         float edl_strength, int edl_px, unsigned char* __restrict__ rgb,
                                                         float* __restrict__ depth, int32_t* __restrict__ ids) {
    const int64_t total = (int64_t)V * H * W, step = (int64_t)gridDim.x * RS_BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; p < total; p += step) {
        const unsigned long long key = fb[p];
        if (key == RS_BG) {
            if (depth) depth[p] = __uint_as_float(0x7f800000u);
            if (ids) ids[p] = -1;
            if (rgb) { rgb[3 * p] = 255; rgb[3 * p + 1] = 255; rgb[3 * p + 2] = 255; }
            continue;
        }
        const float z = __uint_as_float((unsigned)(key >> 32));
        const unsigned id = (unsigned)(key & 0xffffffffull);
        if (depth) depth[p] = z;
        if (ids) ids[p] = (int32_t)id;
        if (!rgb) continue;
        float r, g, b;
        rs_colour(I, id, r, g, b);
        if (edl_strength > 0.0f) {
            const int x = (int)(p % W), y = (int)((p / W) % H);
            const int64_t e = edl_px;
            const float lz = log2f(z);
            float acc = 0.0f;
            const bool in[4] = {x - e >= 0, x + e < W, y - e >= 0, y + e < H};
            const int64_t at[4] = {p - e, p + e, p - e * W, p + e * W};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!in[k]) continue;
                const unsigned long long nb = fb[at[k]];
                if (nb == RS_BG) continue;
                acc += fmaxf(0.0f, lz - log2f(__uint_as_float((unsigned)(nb >> 32))));
            }
            const float shade = expf(-edl_strength * acc);
            r = r * shade; g = g * shade; b = b * shade;
        }
        rgb[3 * p] = rs_to8(r); rgb[3 * p + 1] = rs_to8(g); rgb[3 * p + 2] = rs_to8(b);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct RsWorkspace {
    unsigned long long* fb;
    unsigned* q_count;
    unsigned long long* queue;
    int64_t bytes;
};

static RsWorkspace rs_carve(void* ws, int64_t ws_bytes, int V, int H, int W) {
    StArena a(ws, ws_bytes);
    RsWorkspace r;
    r.fb = a.take<unsigned long long>((int64_t)V * H * W);
    r.q_count = a.take<unsigned>(1);
    r.queue = a.take<unsigned long long>(RS_QUEUE);
    r.bytes = a.used;
    if (!a.ok()) r.fb = nullptr;
    return r;
}

static bool rs_view_ok(int V, int H, int W) {
    return V >= 1 && V <= 65536 && H >= 1 && W >= 1 && H <= RS_MAX_DIM && W <= RS_MAX_DIM;
}

#define RS_REQUIRE_VIEW(what)                                                                                              \
    ST_REQUIRE(rs_view_ok(V, H, W), what ": 1 <= V <= 65536 and 1 <= W, H <= %d (got V %d, H %d, W %d)", RS_MAX_DIM, V, H, W)

#define RS_TAKE_WORKSPACE(what)                                                                                            \
    const RsWorkspace R = rs_carve(ws, ws_bytes, V, H, W);                                                                 \
    if (!ws || !R.fb) {                                                                                                    \
        st_set_error(what ": workspace too small (%lld < %lld)", (long long)(ws ? ws_bytes : 0), (long long)R.bytes);     \
        return ST_ERR_WORKSPACE;                                                                                           \
    }

// -1 for a view the calls refuse
extern "C" int64_t st_render_workspace_bytes(int V, int H, int W) {
    if (!rs_view_ok(V, H, W)) return -1;
    return rs_carve(nullptr, 0, V, H, W).bytes;
}

extern "C" int st_render_clear(int V, int H, int W, void* ws, int64_t ws_bytes, void* stream_) {
    RS_REQUIRE_VIEW("render clear");
    RS_TAKE_WORKSPACE("render clear");
    (void)hipMemsetAsync(R.fb, 0xff, (size_t)V * H * W * sizeof(unsigned long long), (hipStream_t)stream_);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

static bool rs_ids_ok(int64_t n, int64_t id_base) { return n >= 0 && id_base >= 0 && id_base + n < (1ll << 31); }

extern "C" int st_render_points(const float* xyz, const float* radius, int64_t n, int64_t id_base, float point_px, const float* cams,
                                int V, int H, int W, float near, void* ws, int64_t ws_bytes, void* stream_) {
    RS_REQUIRE_VIEW("render points");
    ST_REQUIRE(rs_ids_ok(n, id_base), "render points: ids [%lld, %lld + %lld) must stay below 2^31", (long long)id_base,
               (long long)id_base, (long long)n);
    ST_REQUIRE(n == 0 || xyz, "render points: null xyz with %lld points", (long long)n);
    ST_REQUIRE(cams, "render points: null cameras");
    ST_REQUIRE(near > 0.0f && near <= RS_FLT_MAX, "render points: near must be positive and finite (got %g)", (double)near);
    ST_REQUIRE(point_px >= 0.0f && point_px <= RS_FLT_MAX, "render points: point_px must be finite and >= 0 (got %g)", (double)point_px);
    RS_TAKE_WORKSPACE("render points");
    if (n == 0) return ST_OK;
    hipLaunchKernelGGL(k_rs_points, dim3((unsigned)st_div_up(n, RS_BLOCK)), dim3(RS_BLOCK), 0, (hipStream_t)stream_, xyz, radius, n,
                       (unsigned)id_base, point_px, cams, V, H, W, near, R.fb);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_render_segments(const float* a, const float* b, const float* r1, const float* r2, int64_t m, int64_t id_base,
                                  float min_px, const float* cams, int V, int H, int W, float near, void* ws, int64_t ws_bytes,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RS_REQUIRE_VIEW("render segments");
    ST_REQUIRE(rs_ids_ok(m, id_base), "render segments: ids [%lld, %lld + %lld) must stay below 2^31", (long long)id_base,
               (long long)id_base, (long long)m);
    ST_REQUIRE(m == 0 || (a && b && r1 && r2), "render segments: null input with %lld segments", (long long)m);
    ST_REQUIRE(cams, "render segments: null cameras");
    ST_REQUIRE(near > 0.0f && near <= RS_FLT_MAX, "render segments: near must be positive and finite (got %g)", (double)near);
    ST_REQUIRE(min_px >= 0.0f && min_px <= RS_FLT_MAX, "render segments: min_px must be finite and >= 0 (got %g)", (double)min_px);
    RS_TAKE_WORKSPACE("render segments");
    if (m == 0) return ST_OK;
    (void)hipMemsetAsync(R.q_count, 0, sizeof(unsigned), stream);
    hipLaunchKernelGGL(k_rs_segments_small, dim3((unsigned)st_div_up(m, RS_BLOCK)), dim3(RS_BLOCK), 0, stream, a, b, r1, r2, m,
                       (unsigned)id_base, min_px, cams, V, H, W, near, R.fb, R.q_count, R.queue);
    const int64_t pairs = m * (int64_t)V;
    const int64_t blocks = st_div_up(pairs < RS_QUEUE ? pairs : RS_QUEUE, RS_BLOCK / 64);
    hipLaunchKernelGGL(k_rs_segments_large, dim3((unsigned)(blocks < RS_LARGE_BLOCKS ? blocks : RS_LARGE_BLOCKS)), dim3(RS_BLOCK), 0,
                       stream, a, b, r1, r2, (unsigned)id_base, min_px, cams, H, W, near, R.fb, (const unsigned*)R.q_count,
                       (const unsigned long long*)R.queue);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_render_resolve(const StRenderItem* items_host, int n_items, int V, int H, int W, float edl_strength, int edl_px,
                                 uint8_t* rgb, float* depth, int32_t* ids, void* ws, int64_t ws_bytes, void* stream_) {
    RS_REQUIRE_VIEW("render resolve");
    ST_REQUIRE(n_items >= 0 && n_items <= RS_MAX_ITEMS, "render resolve: 0 .. %d items (got %d)", RS_MAX_ITEMS, n_items);
    ST_REQUIRE(n_items == 0 || items_host, "render resolve: null item table");
    ST_REQUIRE(edl_strength >= 0.0f && edl_strength <= RS_FLT_MAX, "render resolve: shading strength must be finite and >= 0 (got %g)",
               (double)edl_strength);
    ST_REQUIRE(edl_strength == 0.0f || (edl_px >= 1 && edl_px <= RS_MAX_DIM), "render resolve: 1 <= edl_px <= %d (got %d)", RS_MAX_DIM, edl_px);
    RsItems I;
    memset(&I, 0, sizeof(I));
    I.n = n_items;
    int64_t end = 0;
    for (int k = 0; k < n_items; k++) {
        const StRenderItem& it = items_host[k];
        ST_REQUIRE(it.count >= 0 && end + it.count < (1ll << 31), "render resolve: ids must stay below 2^31 (item %d ends at %lld)", k,
                   (long long)(end + it.count));
        ST_REQUIRE(it.mode >= 0 && it.mode <= 4, "render resolve: item %d has colour mode %d (0 .. 4)", k, it.mode);
        ST_REQUIRE(it.mode == 0 || it.count == 0 || it.data, "render resolve: item %d has a null colour source with %lld ids", k,
                   (long long)it.count);
        ST_REQUIRE(it.mode != 2 || (it.n_classes >= 1 && it.cmap), "render resolve: item %d colours by class without a colour map", k);
        end += it.count;
        I.id_end[k] = (int32_t)end;
        I.mode[k] = it.mode; I.n_classes[k] = it.n_classes; I.data[k] = it.data; I.cmap[k] = it.cmap;
        I.lo[k] = it.lo; I.hi[k] = it.hi;
        for (int c = 0; c < 3; c++) I.rgb[k][c] = it.rgb[c];
    }
    RS_TAKE_WORKSPACE("render resolve");
    if (!rgb && !depth && !ids) return ST_OK;
    if (n_items == 0) I.n = 1;  // one empty item: whatever id the framebuffer holds is owned by nobody
    const int64_t blocks = st_div_up((int64_t)V * H * W, RS_BLOCK);
    hipLaunchKernelGGL(k_rs_resolve, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(RS_BLOCK), 0, (hipStream_t)stream_,
                       (const unsigned long long*)R.fb, V, H, W, I, edl_strength, edl_px, rgb, depth, ids);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
