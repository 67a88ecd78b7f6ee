// st_scan_cast_seg: a virtual terrestrial laser scanner.  Beams of scanners standing in up to ST_MAX_SEG clouds are cast against the
// tubes of their cloud's skeleton; the first hit of every beam becomes a labelled point.  What a scan has and a surface sample
// (synthetic.hip) has not: one side of a stem per position, a density that falls with the square of the range, shadows.
//
// Replaces nothing of the reference (it has no scanner model).  The chip has no ray hardware: vector ALU work over a grid.
//
// SURFACE.  The surface of tube g is the zero set of st_tube.h's residual, |p - (a + clip01(t) ab)| = r(clip01(t)),
// t = dot(p - a, ab) / dot(ab, ab): the side of a right circular frustum for 0 <= t <= 1, the part of the sphere of radius r1
// about a with t <= 0, the part of the sphere of radius r2 about b with t >= 1.  A zero-length tube (dot(ab, ab) == 0) is the
// sphere of radius r1 about a (leaves).  A tube with a non-finite end point or radius, or a negative radius, is never hit.
// A ray p(s) = o + s w.  Its hit is the smallest root s over all pieces of all tubes of its cloud with min_range <= s <= max_range;
// a ray that starts inside a tube therefore returns that tube's far wall.  Winner: the minimum of (bits of s, tube index).
//
// SOLVE (float32, this order, no contraction; dot(u, v) = (ux*vx + uy*vy) + uz*vz, st_tube.h's).  Per ray ww = dot(w, w).
//   ab = b - a, ab2 = dot(ab, ab) (st_tube_record).  mid = a + 0.5*ab;  s0 = dot(mid - o, w);  o' = o + s0*w;  m = o' - a.
//   The origin moved to the closest approach first: solved from o the quadratics lose 1 to 2 mm to cancellation at 5 m.
//   quad(A, B, C): disc = B*B - A*C; refused unless disc >= 0; q = -(B + copysign(sqrtf(disc), B)); roots q / A and C / q.
//   sphere a:  quad(ww, dot(m, w), dot(m, m) - r1*r1);  valid root: t <= 0 (no condition for a zero-length tube, and no other piece)
//   sphere b:  n = m - ab;  quad(ww, dot(n, w), dot(n, n) - r2*r2);  valid root: t >= 1
//   side:      t0 = dot(m, ab) / ab2, t1 = dot(w, ab) / ab2;  P = m - t0*ab, Q = w - t1*ab;  dr = r2 - r1, R = r1 + t0*dr, D = t1*dr
//              quad(dot(Q, Q) - D*D, dot(P, Q) - R*D, dot(P, P) - R*R);  valid root: 0 <= t <= 1
//   with t = t0 + s'*t1 of a root s'.  Every root gives s = (s0 + s') + 0 (the + 0 turns -0 into +0) and must satisfy
//   min_range <= s <= max_range and the box rule: x = m + s'*w lies in [min(0, ab_k) - e, max(0, ab_k) + e] on every axis k,
//   e = max(r1, r2) + tau, tau = 2^-10 * (max_k |ab_k| + max(r1, r2)).  In exact arithmetic every root on the surface passes the
//   box rule; it is there so that a root the rounding has thrown far off the tube (a grazing ray on a long tube) is refused in
//   BOTH forms instead of being met by one and not the other.  The tube's s is the smallest valid one; comparisons with NaN fail.
//   Ray k of a scanner is beam (k / n_el, k % n_el): az = az0 + (float)i*daz, el = el0 + (float)j*del,
//   w = (cosf(el)*cosf(az), cosf(el)*sinf(az), sinf(el)).
//   Hit point h = o + s*w per axis (a product, a sum).  Noise: n = the first normal of Box-Muller on words 0, 1 of Philox4x32-10
//   with key = the scanner's seed and counter (k, 0, 0, 0), synthetic.hip's conventions; d = range_noise*n; xyz = h + d*w.
//   Medial vector: st_tube.h's pair at h (t = 0 for a zero-length tube), q - p; zero for a leaf.
//
// Form 1, dense: one ray per lane, the tubes of the clouds a workgroup's rays belong to staged through LDS (st_tube_sweep); a lane
//   takes a tube only inside its own cloud's range.  The yardstick of the grid form, and the path for small tables.
// Form 2, grid: per cloud a uniform grid; tube g is entered into every cell that the box of its axis, inflated by
//   max(r1, r2) + tau_g + margin, margin = cell / 16 + 2^-19 * M, overlaps (count, scan, fill: an own copy of segment.hip's steps,
//   because the inflation differs and segment's bits must not move).  M = the largest |coordinate| of a tube box or of a scanner
//   of the cloud; the cell is kept >= 2^-14 M.  A ray clips itself to the grid box, walks the cells front to back (3D-DDA) and
//   tests the tubes each cell lists.  Why the dense winner T (its s* the overall minimum) is always met:
//     (1) Position, not parameter.  The walk keeps integer cell indices; the parameter at which it leaves cell i along axis k is
//         formed afresh at every step, (lo_k + (float)(i_k [+ 1]) * cell - o_k) / w_k, never accumulated.  Its error e_s may be
//         large when w_k is small, but e_s * |w_k|, the distance of p_k from the plane at that moment, is a few units in the last
//         place of M.  So for every s between the start and the exit parameter of step n, p(s) is, on every axis, within
//         eps <= 2^-21 M of the cell of some step j <= n.  The start cell, floorf((p_k - lo_k) / cell) clamped, is off by at most
//         the same eps (two roundings, <= 1024 cells per axis: 2^-12 cell).
//     (2) The box rule puts p(s*) within tau_T of T's box [axis +- max(r1, r2)], up to the roundings of x against o + s w: a few
//         units in the last place of M.  So p(s*) is inside T's inflated box shrunk by margin - 2^-20 M >= cell/16 + 2^-20 M; with
//         (1), and eps / cell <= 2^-7 < 1/16 - 2^-12, T is listed in the cell of that step j (the listing's own cell arithmetic
//         is the monotone, clamped one of the start cell).
//     (3) The grid box is the union of the inflated boxes, so p(s*) is margin inside it: the computed slab interval [sa, sb] of
//         the ray against the grid box contains s*, a ray whose interval is empty has no hit (rays that miss the box), and a ray
//         that starts inside the box has sa < min_range and starts its walk at min_range in its own cell.
//     (4) A direction component that is exactly 0 never steps on its axis (exit parameter +inf) and clips by o_k alone.
//     (5) The walk stops when its best s is strictly below the exit parameter of the step (everything not met has s* beyond it,
//         by (1) and (2); an equal s* with a lower index has s* < exit as well and was met), when the exit lies beyond
//         min(sb, max_range), or when it leaves the grid.  It takes at most dim_x + dim_y + dim_z steps.
//   A cloud whose coordinates exceed 1e18, or whose lists do not fit, is swept tube by tube.  The cell size changes the speed only.
// Form 0, auto: the grid from SC_AUTO_GRID_M tubes per cloud on (tools/bench_scan.py sweeps the tube count; DESIGN.md "Dataset:
//   scanned trees" has the numbers behind the threshold).
// Wavefront shape: a wavefront takes a patch of 8 x 8 beams in (az, el), not 64 along one axis, so that its rays walk the same
//   cells; the gain is not measured.  Per-ray outputs are indexed by ray, whatever lane computed them.
// Compaction: hit flags, prims.hip's exclusive scan, one pass that writes hit j of ray order: the same order in every run.
// Enqueue-only: no allocation, no read-back, no wait.  The scanner table is a HOST array: it travels as kernel arguments, which is
// what lets the call check it and still not wait.
#include "smarttree_hip.h"  // StScanner, ST_SCAN_MAX_SCANNERS, and the declarations of the entry points below
#include "st_common.h"
#include "st_grid.h"
#include "st_philox.h"
#include "st_tube.h"

#define SC_BLOCK 256
#define SC_TILE 512
#define SC_NONE 0x7f800001u  // "no hit": just above the bits of +inf
#define SC_MAX_DIM 1024
#define SC_AUTO_GRID_M 32    // both forms cost 0.2 ms per 1M beams at 21 tubes, the grid wins clearly from 57 (profiles/scan_bench.json)
#define SC_PLAN_ROUNDS 96
#define SC_PUT 32            // scanners per argument block (2.3 KB of the 4 KB a launch carries): a table of S scanners costs
                             // ceil((S + 1) / 32) tiny launches, 129 at ST_SCAN_MAX_SCANNERS -- the price of checking it on the host
                             // and still not waiting; a ring is 3 to 8 scanners, a batch of 64 clouds a few hundred

struct ScScanner {  // device record; record S is a sentinel that carries the totals
    float pos[3];
    float az0, daz, el0, del;
    float smin, smax, noise;
    int32_t n_az, n_el, cloud;
    uint32_t seed_lo, seed_hi;
    int32_t ray_off, patch_off, patches_el;
};
struct ScPut { ScScanner rec[SC_PUT]; int32_t first, count; };

struct ScCloud {  // 64 bytes; record s of a grid call's workspace is cloud s's plan
    float lo[3];
    float cell;
    int dim[3];
    int sweep;
    int64_t cell_base, cell_cap, entry_cap;
    float mag, margin;
};
static_assert(sizeof(ScCloud) == 64, "smart_tree_amd/scan.py:grid_plan and the tests read this record from the head of the workspace");

// ---------------------------------------------------------------------------------------- the pair ---
__device__ __forceinline__ bool sc_tube_ok(const float* a, const float* b, const float* r1, const float* r2, int64_t g) {
    return st_finite(a[3 * g]) && st_finite(a[3 * g + 1]) && st_finite(a[3 * g + 2]) && st_finite(b[3 * g]) && st_finite(b[3 * g + 1]) &&
           st_finite(b[3 * g + 2]) && st_finite(r1[g]) && st_finite(r2[g]) && r1[g] >= 0.0f && r2[g] >= 0.0f;
}
// st_tube.h's record; a tube that is never hit gets NaN radii, and with them no root passes a comparison
__device__ __forceinline__ void sc_tube_record(const float* a, const float* b, const float* r1, const float* r2, int64_t g, float4* ta,
                                               float4* tb, float* tab2, int64_t j) {
    const bool ok = sc_tube_ok(a, b, r1, r2, g);
    st_tube_record(a, b, r1, r2, g, ta, tb, tab2, j);
    if (!ok) { ta[j].w = __uint_as_float(0x7fc00000u); tb[j].w = __uint_as_float(0x7fc00000u); }
}

struct ScRay {
    float ox, oy, oz, wx, wy, wz, ww, smin, smax;
};

struct ScRoots { float lo, hi; };
__device__ __forceinline__ ScRoots sc_quad(float A, float B, float C) {
    const float nan = __uint_as_float(0x7fc00000u);
    ScRoots r = {nan, nan};
    const float bb = B * B, ac = A * C;
    const float disc = bb - ac;
    if (disc >= 0.0f) {
        const float q = -(B + copysignf(sqrtf(disc), B));
        r.lo = q / A;
        r.hi = C / q;
    }
    return r;
}

// One root s' of piece `piece` (0: sphere a, 1: side, 2: sphere b, 3: the sphere of a zero-length tube) offered to the tube's best.
__device__ __forceinline__ void sc_offer_root(float sp, int piece, const ScRay& r, float s0, float mx, float my, float mz, float t0,
                                              float t1, float4 B, float e, float* best) {
    float t = sp * t1;
    t = t0 + t;
    const bool t_ok = piece == 3 || (piece == 0 && t <= 0.0f) || (piece == 1 && t >= 0.0f && t <= 1.0f) || (piece == 2 && t >= 1.0f);
    float s = s0 + sp;
    s = s + 0.0f;
    float x = sp * r.wx, y = sp * r.wy, z = sp * r.wz;
    x = mx + x; y = my + y; z = mz + z;
    const bool box = x >= fminf(0.0f, B.x) - e && x <= fmaxf(0.0f, B.x) + e && y >= fminf(0.0f, B.y) - e && y <= fmaxf(0.0f, B.y) + e &&
                     z >= fminf(0.0f, B.z) - e && z <= fmaxf(0.0f, B.z) + e;
    if (t_ok && box && s >= r.smin && s <= r.smax && s < *best) *best = s;
}

// The tube's s as the key an unsigned minimum works on: the bits of s (s >= +0), SC_NONE without a hit.
__device__ __forceinline__ unsigned sc_hit(const ScRay& r, float4 A, float4 B, float ab2) {
    float midx = 0.5f * B.x, midy = 0.5f * B.y, midz = 0.5f * B.z;
    midx = A.x + midx; midy = A.y + midy; midz = A.z + midz;
    const float s0 = st_dot3(midx - r.ox, midy - r.oy, midz - r.oz, r.wx, r.wy, r.wz);
    float mx = s0 * r.wx, my = s0 * r.wy, mz = s0 * r.wz;
    mx = r.ox + mx; my = r.oy + my; mz = r.oz + mz;
    mx = mx - A.x; my = my - A.y; mz = mz - A.z;
    const float rmax = fmaxf(A.w, B.w);
    const float e = rmax + 9.765625e-4f * (fmaxf(fmaxf(fabsf(B.x), fabsf(B.y)), fabsf(B.z)) + rmax);
    float best = __uint_as_float(0x7f800000u);  // +inf itself never passes the box rule
    const float mw = st_dot3(mx, my, mz, r.wx, r.wy, r.wz), mm = st_dot3(mx, my, mz, mx, my, mz);
    const ScRoots sa = sc_quad(r.ww, mw, mm - A.w * A.w);
    if (ab2 == 0.0f) {
        sc_offer_root(sa.lo, 3, r, s0, mx, my, mz, 0.0f, 0.0f, B, e, &best);
        sc_offer_root(sa.hi, 3, r, s0, mx, my, mz, 0.0f, 0.0f, B, e, &best);
    } else {
        const float t0 = st_dot3(mx, my, mz, B.x, B.y, B.z) / ab2, t1 = st_dot3(r.wx, r.wy, r.wz, B.x, B.y, B.z) / ab2;
        sc_offer_root(sa.lo, 0, r, s0, mx, my, mz, t0, t1, B, e, &best);
        sc_offer_root(sa.hi, 0, r, s0, mx, my, mz, t0, t1, B, e, &best);
        const float nx = mx - B.x, ny = my - B.y, nz = mz - B.z;
        const ScRoots sb = sc_quad(r.ww, st_dot3(nx, ny, nz, r.wx, r.wy, r.wz), st_dot3(nx, ny, nz, nx, ny, nz) - B.w * B.w);
        sc_offer_root(sb.lo, 2, r, s0, mx, my, mz, t0, t1, B, e, &best);
        sc_offer_root(sb.hi, 2, r, s0, mx, my, mz, t0, t1, B, e, &best);
        float px = t0 * B.x, py = t0 * B.y, pz = t0 * B.z;
        px = mx - px; py = my - py; pz = mz - pz;
        float qx = t1 * B.x, qy = t1 * B.y, qz = t1 * B.z;
        qx = r.wx - qx; qy = r.wy - qy; qz = r.wz - qz;
        const float dr = B.w - A.w;
        float R = t0 * dr;
        R = A.w + R;
        const float D = t1 * dr;
        const ScRoots sc = sc_quad(st_dot3(qx, qy, qz, qx, qy, qz) - D * D, st_dot3(px, py, pz, qx, qy, qz) - R * D,
                                   st_dot3(px, py, pz, px, py, pz) - R * R);
        sc_offer_root(sc.lo, 1, r, s0, mx, my, mz, t0, t1, B, e, &best);
        sc_offer_root(sc.hi, 1, r, s0, mx, my, mz, t0, t1, B, e, &best);
    }
    return best < __uint_as_float(0x7f800000u) ? __float_as_uint(best) : SC_NONE;
}

// ---------------------------------------------------------------------------------------- the rays ---
// the scanner that owns patch p (by patch_off) or ray i (by ray_off): the last one whose offset is <= the index
template <bool BY_PATCH>
__device__ __forceinline__ int sc_find(const ScScanner* sc, int S, int64_t i) {
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)(BY_PATCH ? sc[mid].patch_off : sc[mid].ray_off) <= i) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ ScRay sc_ray(const ScScanner& c, int iaz, int iel) {
    float az = (float)iaz * c.daz, el = (float)iel * c.del;
    az = c.az0 + az;
    el = c.el0 + el;
    const float ce = cosf(el), se = sinf(el), ca = cosf(az), sa = sinf(az);
    ScRay r;
    r.ox = c.pos[0]; r.oy = c.pos[1]; r.oz = c.pos[2];
    r.wx = ce * ca; r.wy = ce * sa; r.wz = se;
    r.ww = st_dot3(r.wx, r.wy, r.wz, r.wx, r.wy, r.wz);
    r.smin = c.smin; r.smax = c.smax;
    return r;
}
// Lane `lane` of patch `patch`: its scanner, its beam and its ray index; false for a lane outside the window.
__device__ __forceinline__ bool sc_lane(const ScScanner* sc, int S, int64_t patch, int lane, int* s_out, int64_t* ray, ScRay* r) {
    const int s = sc_find<true>(sc, S, patch);
    *s_out = s;
    const ScScanner c = sc[s];
    const int local = (int)(patch - c.patch_off);
    const int iaz = (local / c.patches_el) * 8 + (lane >> 3), iel = (local % c.patches_el) * 8 + (lane & 7);
    if (iaz >= c.n_az || iel >= c.n_el) return false;
    *ray = (int64_t)c.ray_off + (int64_t)iaz * c.n_el + iel;
    *r = sc_ray(c, iaz, iel);
    return true;
}
__device__ __forceinline__ void sc_store(int64_t ray, const ScRay& r, unsigned key, int best, float* dir, float* range, int32_t* tube,
                                         uint32_t* flag) {
    const bool hit = key != SC_NONE;
    if (dir) { dir[3 * ray] = r.wx; dir[3 * ray + 1] = r.wy; dir[3 * ray + 2] = r.wz; }
    range[ray] = hit ? __uint_as_float(key) : __uint_as_float(0x7f800000u);
    tube[ray] = hit ? best : -1;
    flag[ray] = hit ? 1u : 0u;
}

__global__ void __launch_bounds__(64) k_sc_put(ScPut p, ScScanner* sc) {
    const int j = threadIdx.x;
    if (j < p.count) sc[p.first + j] = p.rec[j];
}

// ------------------------------------------------------------------------------------ form 1: dense ---
__global__ void __launch_bounds__(SC_BLOCK) k_sc_dense(const ScScanner* __restrict__ sc, int S, int64_t n_patches,
                                                       const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ r1, const float* __restrict__ r2, int64_t m,
                                                       const int32_t* __restrict__ tube_seg_off, float* dir, float* range, int32_t* tube,
                                                       uint32_t* flag) {
    __shared__ float4 ta[SC_TILE], tb[SC_TILE];
    __shared__ float tab2[SC_TILE];
    const int64_t p_first = (int64_t)blockIdx.x * (SC_BLOCK / 64);
    const int64_t p_last = p_first + SC_BLOCK / 64 <= n_patches ? p_first + SC_BLOCK / 64 - 1 : n_patches - 1;
    const int64_t patch = p_first + (threadIdx.x >> 6);
    int64_t t_begin = 0, t_end = m;
    if (tube_seg_off) {
        t_begin = tube_seg_off[sc[sc_find<true>(sc, S, p_first)].cloud];
        t_end = tube_seg_off[sc[sc_find<true>(sc, S, p_last)].cloud + 1];
    }
    int s = 0;
    int64_t ray = 0;
    ScRay r = {};
    const bool live = patch < n_patches && sc_lane(sc, S, patch, threadIdx.x & 63, &s, &ray, &r);
    int lo = 0;
    unsigned cnt = (unsigned)m;  // the lane's own range: tube g counts iff (unsigned)(g - lo) < cnt
    if (live && tube_seg_off) { lo = tube_seg_off[sc[s].cloud]; cnt = (unsigned)(tube_seg_off[sc[s].cloud + 1] - lo); }
    unsigned key = SC_NONE;
    int best = -1;
    st_tube_sweep<SC_BLOCK, SC_TILE>(
        t_begin, t_end, live, [&](int64_t g, int j) { sc_tube_record(a, b, r1, r2, g, ta, tb, tab2, j); },
        [&](int j, int g) {
            const unsigned k = sc_hit(r, ta[j], tb[j], tab2[j]);
            if (k < key && (unsigned)(g - lo) < cnt) { key = k; best = g; }  // ascending g: a tie keeps the lower index
        });
    if (live) sc_store(ray, r, key, best, dir, range, tube, flag);
}

// ------------------------------------------------------------------------------------- form 2: grid ---
// tau_g and the box of tube g's axis inflated by max(r1, r2) + tau_g + margin; false for a tube that is never hit
__device__ __forceinline__ bool sc_box(const float* a, const float* b, const float* r1, const float* r2, int64_t g, float margin, float* lo,
                                       float* hi) {
    if (!sc_tube_ok(a, b, r1, r2, g)) return false;
    const float rmax = fmaxf(r1[g], r2[g]);
    float ext = 0.0f;
    for (int k = 0; k < 3; k++) ext = fmaxf(ext, fabsf(b[3 * g + k] - a[3 * g + k]));
    const float infl = rmax + 9.765625e-4f * (ext + rmax) + margin;
    for (int k = 0; k < 3; k++) {
        lo[k] = fminf(a[3 * g + k], b[3 * g + k]) - infl;
        hi[k] = fmaxf(a[3 * g + k], b[3 * g + k]) + infl;
    }
    return true;
}
__device__ __forceinline__ int sc_axis(float v, float lo, float cell, int dim) {  // clamped as a float, monotone in v
    float c = floorf((v - lo) / cell);
    c = fminf(fmaxf(c, 0.0f), (float)(dim - 1));
    return (int)c;
}
__device__ __forceinline__ float sc_margin(float cell, float mag) { return cell * 0.0625f + 1.9073486e-6f * mag; }

// One workgroup per cloud: the box of the tubes' boxes, the cell size and the grid's shape.
__global__ void __launch_bounds__(SC_BLOCK) k_sc_plan(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                      const int32_t* tube_seg_off, const ScScanner* sc, int S, int cells_per_tube,
                                                      int entries_per_tube, ScCloud* clouds) {
    __shared__ float s_lo[3][SC_BLOCK], s_hi[3][SC_BLOCK], s_ext[SC_BLOCK], s_mag[SC_BLOCK];
    __shared__ unsigned s_cnt[SC_BLOCK];
    __shared__ unsigned long long s_sum[SC_BLOCK];
    __shared__ float r_lo[3], r_hi[3], g_lo[3], g_hi[3], g_cell, g_mag;
    __shared__ int g_dim[3], g_state;  // 0: try this cell size, 1: it fits, 2: give up (sweep)
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = tube_seg_off ? tube_seg_off[s] : 0, t1 = tube_seg_off ? tube_seg_off[s + 1] : m;
    const int64_t cell_base = (int64_t)cells_per_tube * t0 + 64 * (int64_t)s;
    const int64_t cell_cap = (int64_t)cells_per_tube * (t1 - t0) + 64, entry_cap = (int64_t)entries_per_tube * (t1 - t0) + 64;
    const float big = 3.4028234e38f;
    float lo[3] = {big, big, big}, hi[3] = {-big, -big, -big}, ext = 0.0f, mag = 0.0f;
    unsigned cnt = 0u;
    for (int64_t g = t0 + tid; g < t1; g += SC_BLOCK) {
        float bl[3], bh[3];
        if (!sc_box(a, b, r1, r2, g, 0.0f, bl, bh)) continue;
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], bl[k]);
            hi[k] = fmaxf(hi[k], bh[k]);
            mag = fmaxf(mag, fmaxf(fabsf(bl[k]), fabsf(bh[k])));
        }
        ext += fmaxf(fmaxf(bh[0] - bl[0], bh[1] - bl[1]), bh[2] - bl[2]);
        cnt++;
    }
    for (int j = tid; j < S; j += SC_BLOCK)
        if (sc[j].cloud == s) mag = fmaxf(mag, fmaxf(fmaxf(fabsf(sc[j].pos[0]), fabsf(sc[j].pos[1])), fabsf(sc[j].pos[2])));
    for (int k = 0; k < 3; k++) { s_lo[k][tid] = lo[k]; s_hi[k][tid] = hi[k]; }
    s_ext[tid] = ext; s_mag[tid] = mag; s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        float e = 0.0f, mg = 0.0f;
        unsigned c = 0u;
        for (int k = 0; k < 3; k++) { r_lo[k] = big; r_hi[k] = -big; }
        for (int j = 0; j < SC_BLOCK; j++) {
            for (int k = 0; k < 3; k++) { r_lo[k] = fminf(r_lo[k], s_lo[k][j]); r_hi[k] = fmaxf(r_hi[k], s_hi[k][j]); }
            e += s_ext[j]; mg = fmaxf(mg, s_mag[j]); c += s_cnt[j];
        }
        g_mag = mg;
        g_state = 0;
        if (c == 0u) {  // no tube that can be hit: one empty cell
            for (int k = 0; k < 3; k++) { r_lo[k] = 0.0f; r_hi[k] = 0.0f; }
            g_cell = 1.0f;
            g_mag = fminf(mg, 1.0e18f);
        } else if (!(mg <= 1.0e18f)) {
            g_state = 2;
            g_cell = 1.0f;
        } else {
            g_cell = fmaxf(fmaxf(e / (float)c, mg * 6.1035156e-5f), 1.0e-6f);  // the mean extent; >= 2^-14 M
        }
    }
    __syncthreads();
    for (int round = 0; round < SC_PLAN_ROUNDS; round++) {
        if (g_state != 0) break;  // (the same in every lane: read after a barrier, written before the next)
        const float cell = g_cell, margin = sc_margin(cell, g_mag);
        if (tid < 3) {
            g_lo[tid] = r_lo[tid] - margin;
            g_hi[tid] = r_hi[tid] + margin;
            float d = floorf((g_hi[tid] - g_lo[tid]) / cell) + 1.0f;
            g_dim[tid] = (int)fminf(fmaxf(d, 1.0f), (float)SC_MAX_DIM);
        }
        __syncthreads();
        unsigned long long sum = 0ull;  // an upper bound of the entries this cell size makes
        for (int64_t g = t0 + tid; g < t1; g += SC_BLOCK) {
            float bl[3], bh[3];
            if (!sc_box(a, b, r1, r2, g, margin, bl, bh)) continue;
            unsigned long long p = 1ull;
            for (int k = 0; k < 3; k++) p *= (unsigned long long)fminf((float)g_dim[k], floorf((bh[k] - bl[k]) / cell) + 3.0f);
            sum += p;
        }
        s_sum[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            unsigned long long total = 0ull;
            for (int j = 0; j < SC_BLOCK; j++) total += s_sum[j];
            const bool dims_ok = (g_hi[0] - g_lo[0]) / cell < (float)SC_MAX_DIM && (g_hi[1] - g_lo[1]) / cell < (float)SC_MAX_DIM &&
                                 (g_hi[2] - g_lo[2]) / cell < (float)SC_MAX_DIM;
            const int64_t ncell = (int64_t)g_dim[0] * g_dim[1] * g_dim[2];
            if (dims_ok && ncell <= cell_cap && total <= (unsigned long long)entry_cap) g_state = 1;
            else if (round == SC_PLAN_ROUNDS - 1) g_state = 2;
            else g_cell = cell * 1.25f;
        }
        __syncthreads();
    }
    if (tid == 0) {
        ScCloud c;
        const bool sweep = g_state != 1;
        for (int k = 0; k < 3; k++) { c.lo[k] = sweep ? 0.0f : g_lo[k]; c.dim[k] = sweep ? 1 : g_dim[k]; }
        c.cell = g_cell;
        c.sweep = sweep ? 1 : 0;
        c.cell_base = cell_base;
        c.cell_cap = cell_cap;
        c.entry_cap = entry_cap;
        c.mag = g_mag;
        c.margin = sc_margin(g_cell, g_mag);
        clouds[s] = c;
    }
}

// FILL = false: count the tubes of every cell; FILL = true: write them behind the cell's start.  A lane per tube.
template <bool FILL>
__global__ void __launch_bounds__(SC_BLOCK) k_sc_bin(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                     const int32_t* tube_seg_off, int nseg, const ScCloud* clouds, uint32_t* cell_cnt,
                                                     const uint32_t* cell_start, uint32_t* entries, int64_t entry_total) {
    const int64_t g = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (g >= m) return;
    const ScCloud* c = clouds + st_seg_find(tube_seg_off, nseg, g);
    if (c->sweep) return;
    float bl[3], bh[3];
    if (!sc_box(a, b, r1, r2, g, c->margin, bl, bh)) return;
    const int x0 = sc_axis(bl[0], c->lo[0], c->cell, c->dim[0]), x1 = sc_axis(bh[0], c->lo[0], c->cell, c->dim[0]);
    const int y0 = sc_axis(bl[1], c->lo[1], c->cell, c->dim[1]), y1 = sc_axis(bh[1], c->lo[1], c->cell, c->dim[1]);
    const int z0 = sc_axis(bl[2], c->lo[2], c->cell, c->dim[2]), z1 = sc_axis(bh[2], c->lo[2], c->cell, c->dim[2]);
    for (int x = x0; x <= x1; x++)
        for (int y = y0; y <= y1; y++)
            for (int z = z0; z <= z1; z++) {
                const int64_t cell = c->cell_base + ((int64_t)x * c->dim[1] + y) * c->dim[2] + z;
                const uint32_t k = atomicAdd(&cell_cnt[cell], 1u);
                if (FILL) {
                    const int64_t at = (int64_t)cell_start[cell] + k;
                    if (at < entry_total) entries[at] = (uint32_t)g;  // (the plan's bound keeps the lists inside their room)
                }
            }
}

// the tubes as the pair reads them, for the grid form's gathers
__global__ void __launch_bounds__(SC_BLOCK) k_sc_pack(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                      float4* ta, float4* tb, float* tab2) {
    const int64_t g = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (g >= m) return;
    sc_tube_record(a, b, r1, r2, g, ta, tb, tab2, g);
}

__device__ __forceinline__ void sc_offer(const ScRay& r, int g, const float4* ta, const float4* tb, const float* tab2, unsigned* key,
                                         int* best) {
    const unsigned k = sc_hit(r, ta[g], tb[g], tab2[g]);
    if (k < *key || (k == *key && k != SC_NONE && g < *best)) { *key = k; *best = g; }
}
// the parameter at which the ray leaves cell i of one axis (+inf for a component that is exactly 0)
__device__ __forceinline__ float sc_exit(int i, float lo, float cell, float o, float w) {
    if (w == 0.0f) return __uint_as_float(0x7f800000u);
    float plane = (float)(w > 0.0f ? i + 1 : i) * cell;
    plane = lo + plane;
    return (plane - o) / w;
}
// the slab of one axis folded into [sa, sb]; false when the ray cannot be inside
__device__ __forceinline__ bool sc_slab(float o, float w, float lo, float hi, float* sa, float* sb) {
    if (w == 0.0f) return o >= lo && o <= hi;
    const float u = (lo - o) / w, v = (hi - o) / w;
    *sa = fmaxf(*sa, fminf(u, v));
    *sb = fminf(*sb, fmaxf(u, v));
    return true;
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_grid(const ScScanner* __restrict__ sc, int S, int64_t n_patches,
                                                      const ScCloud* __restrict__ clouds, const uint32_t* __restrict__ cell_start,
                                                      const uint32_t* __restrict__ entries, int64_t entry_total,
                                                      const float4* __restrict__ ta, const float4* __restrict__ tb,
                                                      const float* __restrict__ tab2, int64_t m,
                                                      const int32_t* __restrict__ tube_seg_off, float* dir, float* range, int32_t* tube,
                                                      uint32_t* flag) {
    const int64_t patch = (int64_t)blockIdx.x * (SC_BLOCK / 64) + (threadIdx.x >> 6);
    if (patch >= n_patches) return;
    int s = 0;
    int64_t ray = 0;
    ScRay r = {};
    if (!sc_lane(sc, S, patch, threadIdx.x & 63, &s, &ray, &r)) return;
    const int cloud = sc[s].cloud;
    const ScCloud* c = clouds + cloud;
    unsigned key = SC_NONE;
    int best = -1;
    if (c->sweep) {
        const int t0 = tube_seg_off ? tube_seg_off[cloud] : 0, t1 = tube_seg_off ? tube_seg_off[cloud + 1] : (int)m;
        for (int g = t0; g < t1; g++) sc_offer(r, g, ta, tb, tab2, &key, &best);
    } else {
        const int dx = c->dim[0], dy = c->dim[1], dz = c->dim[2];
        const float cell = c->cell, lx = c->lo[0], ly = c->lo[1], lz = c->lo[2];
        float hx = (float)dx * cell, hy = (float)dy * cell, hz = (float)dz * cell;
        hx = lx + hx; hy = ly + hy; hz = lz + hz;
        float sa = r.smin, sb = r.smax;
        bool in = sc_slab(r.ox, r.wx, lx, hx, &sa, &sb);
        in = sc_slab(r.oy, r.wy, ly, hy, &sa, &sb) && in;
        in = sc_slab(r.oz, r.wz, lz, hz, &sa, &sb) && in;
        if (in && sa <= sb) {
            float px = sa * r.wx, py = sa * r.wy, pz = sa * r.wz;
            px = r.ox + px; py = r.oy + py; pz = r.oz + pz;
            int ix = sc_axis(px, lx, cell, dx), iy = sc_axis(py, ly, cell, dy), iz = sc_axis(pz, lz, cell, dz);
            const int stx = r.wx > 0.0f ? 1 : -1, sty = r.wy > 0.0f ? 1 : -1, stz = r.wz > 0.0f ? 1 : -1;
            for (int step = 0; step <= dx + dy + dz; step++) {
                const int64_t at = c->cell_base + ((int64_t)ix * dy + iy) * dz + iz;
                uint32_t u = cell_start[at], e = cell_start[at + 1];
                if ((int64_t)e > entry_total) e = (uint32_t)entry_total;
                for (; u < e; u++) sc_offer(r, (int)entries[u], ta, tb, tab2, &key, &best);
                const float ex = sc_exit(ix, lx, cell, r.ox, r.wx), ey = sc_exit(iy, ly, cell, r.oy, r.wy);
                const float ez = sc_exit(iz, lz, cell, r.oz, r.wz);
                const float out = fminf(fminf(ex, ey), ez);
                if (__uint_as_float(key) < out) break;  // (SC_NONE is a NaN: never less)
                if (!(out <= sb)) break;
                if (ex == out) { ix += stx; if (ix < 0 || ix >= dx) break; }
                else if (ey == out) { iy += sty; if (iy < 0 || iy >= dy) break; }
                else { iz += stz; if (iz < 0 || iz >= dz) break; }
            }
        }
    }
    sc_store(ray, r, key, best, dir, range, tube, flag);
}

// ------------------------------------------------------------------------------------- the hits ---
__global__ void __launch_bounds__(SC_BLOCK) k_sc_finish(const ScScanner* __restrict__ sc, int S, int64_t n_rays,
                                                        const float* __restrict__ range, const int32_t* __restrict__ tube,
                                                        const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                        const float* a, const float* b, const float* r1, const float* r2,
                                                        const uint8_t* __restrict__ tube_class, const int32_t* __restrict__ tube_branch,
                                                        float* xyz, float* mv, float* class_l, int32_t* branch_ids, int32_t* segment,
                                                        int32_t* ray_out, int64_t* n_hits) {
    const int64_t i = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i == 0 && n_hits) n_hits[0] = (int64_t)pos[n_rays];
    if (i >= n_rays || flag[i] == 0u) return;
    const int64_t j = pos[i];
    const int s = sc_find<false>(sc, S, i);
    const ScScanner c = sc[s];
    const uint32_t k = (uint32_t)(i - c.ray_off);
    const ScRay r = sc_ray(c, (int)(k / (uint32_t)c.n_el), (int)(k % (uint32_t)c.n_el));
    const float sr = range[i];
    const int g = tube[i];
    float hx = sr * r.wx, hy = sr * r.wy, hz = sr * r.wz;
    hx = r.ox + hx; hy = r.oy + hy; hz = r.oz + hz;
    const bool leaf = tube_class != nullptr && tube_class[g] != 0;
    if (xyz) {
        const SyWords wd = sy_philox(k, 0u, 0u, 0u, c.seed_lo, c.seed_hi);
        float nrm, unused;
        sy_normal_pair(wd.w0, wd.w1, nrm, unused);
        const float d = c.noise * nrm;
        float nx = d * r.wx, ny = d * r.wy, nz = d * r.wz;
        nx = hx + nx; ny = hy + ny; nz = hz + nz;
        xyz[3 * j] = nx; xyz[3 * j + 1] = ny; xyz[3 * j + 2] = nz;
    }
    if (mv) {
        float vx = 0.0f, vy = 0.0f, vz = 0.0f;
        if (!leaf) {
            float4 A, B;
            float ab2;
            st_tube_record(a, b, r1, r2, g, &A, &B, &ab2, 0);
            const float t = ab2 == 0.0f ? 0.0f : st_tube_t_div(hx, hy, hz, A, B, ab2);
            const StPair<float> p = st_tube_pair_at(t, hx, hy, hz, A, B);
            vx = p.vx; vy = p.vy; vz = p.vz;
        }
        mv[3 * j] = vx; mv[3 * j + 1] = vy; mv[3 * j + 2] = vz;
    }
    if (class_l) class_l[j] = leaf ? 1.0f : 0.0f;
    if (branch_ids) branch_ids[j] = leaf || tube_branch == nullptr ? -1 : tube_branch[g];
    if (segment) segment[j] = g;
    if (ray_out) ray_out[j] = (int32_t)i;
}

// --------------------------------------------------------------------------------------- host ---
struct ScLayout {
    ScScanner* sc;
    float* range;
    int32_t* tube;
    uint32_t *flag, *pos;
    char* rws;
    int64_t rws_bytes;
    ScCloud* clouds;
    float4 *ta, *tb;
    float* tab2;
    uint32_t *cell_cnt, *cell_start, *entries;
    char* sws;
    int64_t cells, entry_total, sws_bytes;
    int cells_per_tube, entries_per_tube;
};

static void sc_layout(StArena& a, int64_t n_rays, int64_t m, int S, int nseg, ScLayout* L) {
    const int64_t mm = m > 0 ? m : 1;
    L->cells_per_tube = (int)st_min64(8, (1ll << 28) / mm > 0 ? (1ll << 28) / mm : 1);
    L->entries_per_tube = (int)st_min64(32, (1ll << 30) / mm > 0 ? (1ll << 30) / mm : 1);
    L->cells = (int64_t)L->cells_per_tube * m + 64 * (int64_t)nseg;
    L->entry_total = (int64_t)L->entries_per_tube * m + 64 * (int64_t)nseg;
    L->clouds = a.take<ScCloud>(ST_MAX_SEG);  // first: tools/bench_scan.py and the tests read the plan from the head of the workspace
    L->sc = a.take<ScScanner>(S + 1);
    L->range = a.take<float>(n_rays);
    L->tube = a.take<int32_t>(n_rays);
    L->flag = a.take<uint32_t>(n_rays + 1);
    L->pos = a.take<uint32_t>(n_rays + 1);
    L->rws_bytes = st_scan_ws_bytes(n_rays + 1);
    L->rws = a.take<char>(L->rws_bytes);
    L->ta = a.take<float4>(m);
    L->tb = a.take<float4>(m);
    L->tab2 = a.take<float>(m);
    L->cell_cnt = a.take<uint32_t>(L->cells + 1);
    L->cell_start = a.take<uint32_t>(L->cells + 1);
    L->entries = a.take<uint32_t>(L->entry_total);
    L->sws_bytes = st_scan_ws_bytes(L->cells + 1);
    L->sws = a.take<char>(L->sws_bytes);
}

static bool sc_sizes_ok(int64_t n_rays, int64_t m, int S, int nseg) {
    return n_rays >= 0 && n_rays < (1ll << 31) - 1 && m >= 0 && m < (1ll << 31) && S >= 0 && S <= ST_SCAN_MAX_SCANNERS && nseg >= 1 &&
           nseg <= ST_MAX_SEG;
}

extern "C" int64_t st_scan_cast_workspace_bytes(int64_t n_rays, int64_t m, int n_scanners, int nseg) {
    if (!sc_sizes_ok(n_rays, m, n_scanners, nseg)) return -1;
    StArena a(nullptr, 0);
    ScLayout L;
    sc_layout(a, n_rays, m, n_scanners, nseg, &L);
    return a.used;
}

extern "C" int st_scan_cast_seg(const float* a, const float* b, const float* r1, const float* r2, int64_t m, const int32_t* tube_seg_off,
                                int nseg, const uint8_t* tube_class, const int32_t* tube_branch, const StScanner* scanners,
                                int n_scanners, const int64_t* ray_off, int form, float* dir, float* range, int32_t* tube, float* xyz,
                                float* medial_vector, float* class_l, int32_t* branch_ids, int32_t* segment, int32_t* ray,
                                int64_t* n_hits, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int S = n_scanners;
    ST_REQUIRE(m >= 0 && m < (1ll << 31), "scan_cast: 0 <= tubes < 2^31 (got %lld)", (long long)m);
    ST_REQUIRE(nseg >= 1 && nseg <= ST_MAX_SEG, "scan_cast: 1 <= clouds per batch <= %d (got %d)", ST_MAX_SEG, nseg);
    ST_REQUIRE(nseg == 1 || tube_seg_off, "scan_cast: %d clouds need the offsets of their tubes", nseg);
    ST_REQUIRE(S >= 0 && S <= ST_SCAN_MAX_SCANNERS, "scan_cast: 0 <= scanners <= %d (got %d)", ST_SCAN_MAX_SCANNERS, S);
    ST_REQUIRE(S == 0 || (scanners && ray_off), "scan_cast: null scanner table or ray offsets");
    ST_REQUIRE(form >= 0 && form <= 2, "scan_cast: form must be 0 (auto), 1 (dense) or 2 (grid), got %d", form);
    ST_REQUIRE(m == 0 || (a && b && r1 && r2), "scan_cast: null tube array");
    int64_t n_rays = 0, n_patches = 0;
    for (int s = 0; s < S; s++) {
        const StScanner& c = scanners[s];
        ST_REQUIRE(c.cloud >= 0 && c.cloud < nseg && (s == 0 || c.cloud >= scanners[s - 1].cloud),
                   "scan_cast: scanner %d stands in cloud %d; clouds are 0 .. %d and may not decrease along the table", s, (int)c.cloud, nseg - 1);
        ST_REQUIRE(c.n_az >= 0 && c.n_el >= 0 && (int64_t)c.n_az * c.n_el < (1ll << 31) - 1, "scan_cast: scanner %d has %d x %d beams", s,
                   (int)c.n_az, (int)c.n_el);
        bool fin = true;
        for (int k = 0; k < 3; k++) fin = fin && fabsf(c.position[k]) <= 3.4028234e38f;
        fin = fin && fabsf(c.az0) <= 3.4028234e38f && fabsf(c.daz) <= 3.4028234e38f && fabsf(c.el0) <= 3.4028234e38f &&
              fabsf(c.del) <= 3.4028234e38f && fabsf(c.range_noise) <= 3.4028234e38f;
        ST_REQUIRE(fin, "scan_cast: scanner %d has a non-finite position, angle or range_noise", s);
        ST_REQUIRE(c.min_range >= 0.0f && c.max_range >= c.min_range, "scan_cast: scanner %d needs 0 <= min_range <= max_range (no NaN)", s);
        ST_REQUIRE(ray_off[s] == n_rays, "scan_cast: ray_off[%d] = %lld, the beams before it are %lld", s, (long long)ray_off[s],
                   (long long)n_rays);
        n_rays += (int64_t)c.n_az * c.n_el;
        n_patches += st_div_up(c.n_az, 8) * st_div_up(c.n_el, 8);
    }
    ST_REQUIRE(S == 0 || ray_off[S] == n_rays, "scan_cast: ray_off[%d] = %lld, the beams are %lld", S, (long long)(S ? ray_off[S] : 0),
               (long long)n_rays);
    ST_REQUIRE(n_rays < (1ll << 31) - 1 && n_patches < (1ll << 31) - 1, "scan_cast: %lld beams in one call (fewer than 2^31 - 1)", (long long)n_rays);
    StArena arena(ws, ws_bytes);
    ScLayout L;
    sc_layout(arena, n_rays, m, S, nseg, &L);
    if (!arena.ok() || !ws) {
        st_set_error("scan_cast: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (nseg == 1) tube_seg_off = nullptr;
    if (n_rays == 0) {
        if (n_hits) (void)hipMemsetAsync(n_hits, 0, sizeof(int64_t), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    // the scanner records, SC_PUT per argument block; record S carries the totals
    {
        ScPut put;
        memset(&put, 0, sizeof(put));
        put.first = 0;
        int64_t rays = 0, patches = 0;
        for (int s = 0; s <= S; s++) {
            ScScanner& d = put.rec[s - put.first];
            memset(&d, 0, sizeof(d));
            d.ray_off = (int32_t)rays;
            d.patch_off = (int32_t)patches;
            d.patches_el = 1;
            if (s < S) {
                const StScanner& c = scanners[s];
                for (int k = 0; k < 3; k++) d.pos[k] = c.position[k];
                d.az0 = c.az0; d.daz = c.daz; d.el0 = c.el0; d.del = c.del;
                d.smin = c.min_range; d.smax = c.max_range; d.noise = c.range_noise;
                d.n_az = c.n_az; d.n_el = c.n_el; d.cloud = c.cloud;
                d.seed_lo = (uint32_t)c.seed; d.seed_hi = (uint32_t)(c.seed >> 32);
                d.patches_el = (int32_t)st_div_up(c.n_el, 8) > 0 ? (int32_t)st_div_up(c.n_el, 8) : 1;
                rays += (int64_t)c.n_az * c.n_el;
                patches += st_div_up(c.n_az, 8) * st_div_up(c.n_el, 8);
            } else {
                d.cloud = nseg - 1;
            }
            if (s - put.first + 1 == SC_PUT || s == S) {
                put.count = s - put.first + 1;
                hipLaunchKernelGGL(k_sc_put, dim3(1), dim3(64), 0, stream, put, L.sc);
                put.first = s + 1;
            }
        }
    }
    float* range_w = range ? range : L.range;
    int32_t* tube_w = tube ? tube : L.tube;
    (void)hipMemsetAsync(L.flag + n_rays, 0, sizeof(uint32_t), stream);
    if (form == 0) form = m / nseg >= SC_AUTO_GRID_M ? 2 : 1;
    if (m == 0) form = 1;  // nothing to bin: the dense loop over no tubes leaves every ray without a hit
    const unsigned blocks = (unsigned)st_div_up(n_patches, SC_BLOCK / 64);
    if (form == 1) {
        hipLaunchKernelGGL(k_sc_dense, dim3(blocks), dim3(SC_BLOCK), 0, stream, (const ScScanner*)L.sc, S, n_patches, a, b, r1, r2, m,
                           tube_seg_off, dir, range_w, tube_w, L.flag);
    } else {
        const unsigned mb = (unsigned)st_div_up(m, SC_BLOCK);
        hipLaunchKernelGGL(k_sc_plan, dim3((unsigned)nseg), dim3(SC_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, (const ScScanner*)L.sc,
                           S, L.cells_per_tube, L.entries_per_tube, L.clouds);
        hipLaunchKernelGGL(k_sc_pack, dim3(mb), dim3(SC_BLOCK), 0, stream, a, b, r1, r2, m, L.ta, L.tb, L.tab2);
        (void)hipMemsetAsync(L.cell_cnt, 0, (size_t)(L.cells + 1) * sizeof(uint32_t), stream);
        hipLaunchKernelGGL((k_sc_bin<false>), dim3(mb), dim3(SC_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, nseg,
                           (const ScCloud*)L.clouds, L.cell_cnt, (const uint32_t*)nullptr, (uint32_t*)nullptr, L.entry_total);
        ST_TRY(st_exclusive_scan_u32(L.cell_cnt, L.cell_start, L.cells + 1, nullptr, L.sws, L.sws_bytes, stream));
        (void)hipMemsetAsync(L.cell_cnt, 0, (size_t)(L.cells + 1) * sizeof(uint32_t), stream);
        hipLaunchKernelGGL((k_sc_bin<true>), dim3(mb), dim3(SC_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, nseg,
                           (const ScCloud*)L.clouds, L.cell_cnt, (const uint32_t*)L.cell_start, L.entries, L.entry_total);
        hipLaunchKernelGGL(k_sc_grid, dim3(blocks), dim3(SC_BLOCK), 0, stream, (const ScScanner*)L.sc, S, n_patches,
                           (const ScCloud*)L.clouds, (const uint32_t*)L.cell_start, (const uint32_t*)L.entries, L.entry_total,
                           (const float4*)L.ta, (const float4*)L.tb, (const float*)L.tab2, m, tube_seg_off, dir, range_w, tube_w, L.flag);
    }
    if (xyz || medial_vector || class_l || branch_ids || segment || ray || n_hits) {
        ST_TRY(st_exclusive_scan_u32(L.flag, L.pos, n_rays + 1, nullptr, L.rws, L.rws_bytes, stream));
        hipLaunchKernelGGL(k_sc_finish, dim3((unsigned)st_div_up(n_rays, SC_BLOCK)), dim3(SC_BLOCK), 0, stream, (const ScScanner*)L.sc, S,
                           n_rays, (const float*)range_w, (const int32_t*)tube_w, (const uint32_t*)L.flag, (const uint32_t*)L.pos, a, b, r1,
                           r2, tube_class, tube_branch, xyz, medial_vector, class_l, branch_ids, segment, ray, n_hits);
    }
    ST_CHECK_LAUNCH();
    return ST_OK;
}
