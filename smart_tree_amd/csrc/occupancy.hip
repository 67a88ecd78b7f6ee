// st_beam_tally_seg: beams walked through voxel grids.  Every beam of a scan -- origin, unit direction, range, +inf when nothing
// came back -- is walked through its grid and tallied per cell: how many beams entered the cell while still free, how many ended
// in it, how many would have passed had they not been stopped before it, and how much free path they spent in it.  From these
// come the state of a cell (unseen, empty, occupied, occluded) and its contact frequency hit / path (plant-area density).
//
// Replaces nothing of the reference (it keeps no beams).  Integer tallies only: the result does not depend on the order of the
// additions, so it is the same in every run, in both forms, and equal to tests/occupancy_oracle.py's numpy restatement.
//
// WALK (float32, every operation its own statement, this order, no contraction).  Beam i of grid g (beam_off[g] <= i < beam_off[g+1])
// has o = origins[origin_idx[i]], w = dir[i], r = range[i].  The grid has lo, cell, dim; hi_k = lo_k + (float)dim_k * cell.
//   BAD (counted in n_bad, touches nothing): origin_idx outside [0, S); a non-finite o_k or w_k; r NaN, -inf or < 0;
//     ww = (wx*wx + wy*wy) + wz*wz outside [0.998, 1.002].
//   f = fminf(r, max_range), the free end.  The beam is a RETURN when r is finite and r <= max_range, else a miss: nothing beyond
//     max_range is known, so a return from beyond it is a beam stopped by max_range like any other.
//   SLABS, from sa = 0, sb = +inf, axes x, y, z (scan.hip's sc_slab): w_k == 0 keeps the interval and needs lo_k <= o_k <= hi_k;
//     otherwise u = (lo_k - o_k) / w_k, v = (hi_k - o_k) / w_k, sa = fmaxf(sa, fminf(u, v)), sb = fminf(sb, fmaxf(u, v)).
//     OUTSIDE (counted in n_outside, touches nothing): a failed axis, !(sa <= sb), or sa = +inf (a quotient that overflowed).
//   A miss with f < sa contributes nothing.  A return with f < sa is behind from its first cell and has no hit cell.
//   FIRST CELL: p_k = o_k + sa * w_k (a product, a sum); i_k = (int)fminf(fmaxf(floorf((p_k - lo_k) / cell), 0), dim_k - 1)
//     (scan.hip's sc_axis: clamped as a float, a NaN becomes 0).  s_in = sa.
//   STEP, at most dim_x + dim_y + dim_z + 1 cells:
//     exit_k = +inf when w_k == 0, else ((lo_k + (float)(w_k > 0 ? i_k + 1 : i_k) * cell) - o_k) / w_k   (sc_exit: formed afresh
//     from the integer index, never accumulated);  out = fminf(fminf(exit_x, exit_y), exit_z);  e = fminf(out, sb).
//     A free beam:  enter += 1;  path += q(fminf(e, f) - s_in);  if f <= e: a return adds hit += 1, names the cell as its hit cell
//       and turns behind (it ends there when the `behind` flag is off); a miss (stopped by max_range) ends.
//     A beam that is behind:  behind += 1  (so the hit cell itself gets none).
//     The beam leaves the grid unless out < sb.  Otherwise it steps on the first axis, x before y before z, whose exit equals out,
//     by +1 or -1 after the sign of w_k; an index outside [0, dim_k) ends the walk; s_in = out.
//   q(d), the chord in units of cell / 65536:  t = fmaxf(d, 0) / cell;  u = t * 65536;  q = (uint64)rintf(fminf(u, 4294967296))
//     (a division, a product, a round to nearest even; the two clamps keep a chord that rounding made negative at 0 and the
//     conversion defined).  A cell crossed with a zero chord still counts as entered.
//
// Form 1, aggregated: one beam per lane.  At every step the lanes of a wavefront that stand in the same cell as the wavefront's
//   first active lane are found by ballot, their counts are popcounts of ballots, their chords a wave reduction; the first lane
//   issues one atomic per field for all of them, every other lane its own.  All beams of a scanner share their first cell and
//   neighbours in ray order share cells for much of their way: that is the contention this form takes off the L2's adders.
// Form 2, plain: one atomic per lane and field.  The same bits (integer sums).
// Form 0, auto: OC_AUTO_FORM (tools/bench_occupancy.py times both; DESIGN.md "Occupancy: beams through voxels" has the table).
// Enqueue-only: no allocation, no read-back, no wait.  The grid table and beam_off are HOST arrays: they travel as kernel
// arguments into the workspace, which is what lets the call check them and still not wait.  The call zeroes its outputs.
#include "smarttree_hip.h"  // StVoxelGrid and the declarations of the entry points below
#include "st_common.h"

#define OC_BLOCK 256
#define OC_MAX_DIM 1024
#define OC_MAX_GRIDS 64  // st_abi_entries(2)
#define OC_AUTO_FORM 1  // the aggregated form: the faster one on the 3-scanner case of profiles/occupancy_bench.json
#define OC_INF 0x7f800000u

struct OcGrid {  // device record; record G is a sentinel whose beam_first is R
    float lo[3];
    float cell;
    int32_t dim[3];
    int32_t beam_first;
    int64_t cell_base;
};
struct OcPut { OcGrid rec[OC_MAX_GRIDS + 1]; int32_t count; };
static_assert(sizeof(OcPut) <= 3072, "the grid table travels as kernel arguments");

__global__ void __launch_bounds__(128) k_oc_put(OcPut p, OcGrid* grids) {
    const int j = threadIdx.x;
    if (j < p.count) grids[j] = p.rec[j];
}

__device__ __forceinline__ bool oc_finite(float v) { return fabsf(v) <= 3.4028234e38f; }
__device__ __forceinline__ int oc_axis(float v, float lo, float cell, int dim) {  // scan.hip's sc_axis
    float c = v - lo;
    c = c / cell;
    c = floorf(c);
    c = fminf(fmaxf(c, 0.0f), (float)(dim - 1));
    return (int)c;
}
__device__ __forceinline__ float oc_exit(int i, float lo, float cell, float o, float w) {  // scan.hip's sc_exit
    if (w == 0.0f) return __uint_as_float(OC_INF);
    float plane = (float)(w > 0.0f ? i + 1 : i) * cell;
    plane = lo + plane;
    plane = plane - o;
    return plane / w;
}
__device__ __forceinline__ bool oc_slab(float o, float w, float lo, float hi, float* sa, float* sb) {  // scan.hip's sc_slab
    if (w == 0.0f) return o >= lo && o <= hi;
    float u = lo - o, v = hi - o;
    u = u / w;
    v = v / w;
    *sa = fmaxf(*sa, fminf(u, v));
    *sb = fminf(*sb, fmaxf(u, v));
    return true;
}
__device__ __forceinline__ unsigned long long oc_q(float d, float cell) {
    float t = fmaxf(d, 0.0f);
    t = t / cell;
    t = t * 65536.0f;
    t = fminf(t, 4294967296.0f);
    return (unsigned long long)rintf(t);
}

struct OcBeam {  // one lane's walk
    float ox, oy, oz, wx, wy, wz;
    float lx, ly, lz, cell, sb, f, s_in;
    int dx, dy, dz, ix, iy, iz, steps;
    int64_t base;
    bool active, free_, ret;
};
struct OcStep {  // what one cell gets from one beam, and how the beam goes on
    int32_t c;   // cell index inside the beam's grid
    unsigned enter, hit, behind;
    unsigned long long q;
    float out;
    bool ends;
};

// the grid that owns beam i: the last record whose beam_first is <= i (an empty grid is never the last such)
__device__ __forceinline__ int oc_find(const OcGrid* g, int G, int64_t i) {
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)g[mid].beam_first <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Set up beam i; counts it as bad or outside where it is.  b->active says whether it walks.
__device__ __forceinline__ void oc_start(int64_t i, const float* origins, int64_t S, const int32_t* origin_idx, const float* dir,
                                         const float* range, const OcGrid* grids, int G, float max_range, int behind, uint32_t* counters,
                                         OcBeam* b) {
    b->active = false;
    const int32_t k = origin_idx[i];
    const float r = range[i];
    const float wx = dir[3 * i], wy = dir[3 * i + 1], wz = dir[3 * i + 2];
    bool good = k >= 0 && (int64_t)k < S && oc_finite(wx) && oc_finite(wy) && oc_finite(wz) && r >= 0.0f;  // (NaN, -inf: not >= 0)
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (good) {
        ox = origins[3 * (int64_t)k]; oy = origins[3 * (int64_t)k + 1]; oz = origins[3 * (int64_t)k + 2];
        good = oc_finite(ox) && oc_finite(oy) && oc_finite(oz);
    }
    const float xx = wx * wx, yy = wy * wy, zz = wz * wz;
    float ww = xx + yy;
    ww = ww + zz;
    good = good && ww >= 0.998f && ww <= 1.002f;
    if (!good) { atomicAdd(&counters[0], 1u); return; }
    const OcGrid g = grids[oc_find(grids, G, i)];
    b->ox = ox; b->oy = oy; b->oz = oz; b->wx = wx; b->wy = wy; b->wz = wz;
    b->lx = g.lo[0]; b->ly = g.lo[1]; b->lz = g.lo[2]; b->cell = g.cell;
    b->dx = g.dim[0]; b->dy = g.dim[1]; b->dz = g.dim[2];
    b->base = g.cell_base;
    float hx = (float)b->dx * b->cell, hy = (float)b->dy * b->cell, hz = (float)b->dz * b->cell;
    hx = b->lx + hx; hy = b->ly + hy; hz = b->lz + hz;
    float sa = 0.0f, sb = __uint_as_float(OC_INF);
    bool in = oc_slab(ox, wx, b->lx, hx, &sa, &sb);
    in = oc_slab(oy, wy, b->ly, hy, &sa, &sb) && in;
    in = oc_slab(oz, wz, b->lz, hz, &sa, &sb) && in;
    if (!(in && sa <= sb && sa <= 3.4028234e38f)) { atomicAdd(&counters[1], 1u); return; }
    b->ret = r <= 3.4028234e38f && r <= max_range;
    b->f = fminf(r, max_range);
    b->sb = sb;
    b->free_ = true;
    if (b->f < sa) {
        if (!b->ret || !behind) return;
        b->free_ = false;
    }
    float px = sa * wx, py = sa * wy, pz = sa * wz;
    px = ox + px; py = oy + py; pz = oz + pz;
    b->ix = oc_axis(px, b->lx, b->cell, b->dx);
    b->iy = oc_axis(py, b->ly, b->cell, b->dy);
    b->iz = oc_axis(pz, b->lz, b->cell, b->dz);
    b->s_in = sa;
    b->steps = 0;
    b->active = true;
}

// what the beam's present cell gets
__device__ __forceinline__ OcStep oc_cell(const OcBeam& b) {
    OcStep s;
    s.c = (int32_t)(((int64_t)b.ix * b.dy + b.iy) * b.dz + b.iz);
    const float ex = oc_exit(b.ix, b.lx, b.cell, b.ox, b.wx), ey = oc_exit(b.iy, b.ly, b.cell, b.oy, b.wy);
    const float ez = oc_exit(b.iz, b.lz, b.cell, b.oz, b.wz);
    s.out = fminf(fminf(ex, ey), ez);
    const float e = fminf(s.out, b.sb);
    s.enter = 0u; s.hit = 0u; s.behind = 0u; s.q = 0ull; s.ends = false;
    if (b.free_) {
        s.enter = 1u;
        const float m = fminf(e, b.f);
        s.q = oc_q(m - b.s_in, b.cell);
        if (b.f <= e) {
            if (b.ret) s.hit = 1u; else s.ends = true;
        }
    } else {
        s.behind = 1u;
    }
    return s;
}

// move on after the cell was tallied
__device__ __forceinline__ void oc_advance(OcBeam* b, const OcStep& s, int behind, int64_t i, int32_t* hit_cell) {
    if (s.hit) {
        if (hit_cell) hit_cell[i] = s.c;
        b->free_ = false;
        if (!behind) { b->active = false; return; }
    }
    if (s.ends || !(s.out < b->sb)) { b->active = false; return; }
    const float ex = oc_exit(b->ix, b->lx, b->cell, b->ox, b->wx), ey = oc_exit(b->iy, b->ly, b->cell, b->oy, b->wy);
    if (ex == s.out) { b->ix += b->wx > 0.0f ? 1 : -1; if (b->ix < 0 || b->ix >= b->dx) b->active = false; }
    else if (ey == s.out) { b->iy += b->wy > 0.0f ? 1 : -1; if (b->iy < 0 || b->iy >= b->dy) b->active = false; }
    else { b->iz += b->wz > 0.0f ? 1 : -1; if (b->iz < 0 || b->iz >= b->dz) b->active = false; }
    b->s_in = s.out;
    b->steps++;
    if (b->steps > b->dx + b->dy + b->dz) b->active = false;
}

__device__ __forceinline__ void oc_add(int64_t at, unsigned n_enter, unsigned n_hit, unsigned n_behind, unsigned long long q,
                                       uint32_t* enter, uint32_t* hit, uint32_t* behind_out, unsigned long long* path) {
    if (n_enter) atomicAdd(&enter[at], n_enter);
    if (n_hit) atomicAdd(&hit[at], n_hit);
    if (n_behind) atomicAdd(&behind_out[at], n_behind);
    if (q) atomicAdd(&path[at], q);
}

template <bool AGG>
__global__ void __launch_bounds__(OC_BLOCK) k_oc_tally(const float* __restrict__ origins, int64_t S, const int32_t* __restrict__ origin_idx,
                                                       const float* __restrict__ dir, const float* __restrict__ range, int64_t R,
                                                       const OcGrid* __restrict__ grids, int G, float max_range, int behind,
                                                       uint32_t* enter, uint32_t* hit, uint32_t* behind_out, unsigned long long* path,
                                                       int32_t* hit_cell, uint32_t* counters) {
    const int64_t i = (int64_t)blockIdx.x * OC_BLOCK + threadIdx.x;
    OcBeam b;
    b.active = false;
    if (i < R) {
        if (hit_cell) hit_cell[i] = -1;
        oc_start(i, origins, S, origin_idx, dir, range, grids, G, max_range, behind, counters, &b);
    }
    if (!AGG) {
        while (b.active) {
            const OcStep s = oc_cell(b);
            oc_add(b.base + s.c, s.enter, s.hit, s.behind, s.q, enter, hit, behind_out, path);
            oc_advance(&b, s, behind, i, hit_cell);
        }
        return;
    }
    // every lane of the wavefront stays in the loop until none is active: the collectives below are reached by all of them
    const int lane = threadIdx.x & 63;
    for (;;) {
        const unsigned long long act = __ballot(b.active);
        if (act == 0ull) break;
        OcStep s = {};
        int64_t at = -1;
        if (b.active) { s = oc_cell(b); at = b.base + s.c; }
        const int first = __ffsll(act) - 1;
        const unsigned at_lo = __shfl((unsigned)(at & 0xffffffffll), first);  // (all cells of a call: fewer than 2^31)
        const bool same = b.active && (unsigned)(at & 0xffffffffll) == at_lo;
        const unsigned long long group = __ballot(same);
        if (__popcll(group) > 1) {  // (the same in every lane)
            const unsigned n_enter = (unsigned)__popcll(__ballot(same && s.enter));
            const unsigned n_hit = (unsigned)__popcll(__ballot(same && s.hit));
            const unsigned n_behind = (unsigned)__popcll(__ballot(same && s.behind));
            unsigned long long q = same ? s.q : 0ull;
            for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d);
            if (lane == first) oc_add(at, n_enter, n_hit, n_behind, q, enter, hit, behind_out, path);
            else if (b.active && !same) oc_add(at, s.enter, s.hit, s.behind, s.q, enter, hit, behind_out, path);
        } else if (b.active) {
            oc_add(at, s.enter, s.hit, s.behind, s.q, enter, hit, behind_out, path);
        }
        if (b.active) oc_advance(&b, s, behind, i, hit_cell);
    }
}

// --------------------------------------------------------------------------------------- host ---
static bool oc_sizes_ok(int64_t n_beams, int n_grids) { return n_beams >= 0 && n_beams < (1ll << 31) && n_grids >= 1 && n_grids <= OC_MAX_GRIDS; }

extern "C" int64_t st_beam_tally_workspace_bytes(int64_t n_beams, int n_grids) {
    if (!oc_sizes_ok(n_beams, n_grids)) return -1;
    StArena a(nullptr, 0);
    a.take<OcGrid>(OC_MAX_GRIDS + 1);
    return a.used;
}

extern "C" int st_beam_tally_seg(const float* origins, int64_t n_origins, const int32_t* origin_idx, const float* dir, const float* range,
                                 int64_t n_beams, const StVoxelGrid* grids, int n_grids, const int64_t* beam_off, float max_range,
                                 int behind, int form, uint32_t* enter, uint32_t* hit, uint32_t* behind_out, uint64_t* path,
                                 int32_t* hit_cell, uint32_t* counters, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int G = n_grids;
    const int64_t R = n_beams;
    ST_REQUIRE(R >= 0 && R < (1ll << 31), "beam_tally: 0 <= beams < 2^31 (got %lld)", (long long)R);
    ST_REQUIRE(G >= 1 && G <= OC_MAX_GRIDS, "beam_tally: 1 <= grids per call <= %d (got %d)", OC_MAX_GRIDS, G);
    ST_REQUIRE(grids && beam_off, "beam_tally: null grid table or beam offsets");
    ST_REQUIRE(n_origins >= 0 && n_origins < (1ll << 31), "beam_tally: 0 <= origins < 2^31 (got %lld)", (long long)n_origins);
    ST_REQUIRE(form >= 0 && form <= 2, "beam_tally: form must be 0 (auto), 1 (aggregated) or 2 (plain), got %d", form);
    ST_REQUIRE(max_range >= 0.0f, "beam_tally: max_range must be >= 0 (+inf allowed, no NaN)");
    ST_REQUIRE(enter && hit && behind_out && path && counters, "beam_tally: null output");
    ST_REQUIRE(R == 0 || (origin_idx && dir && range && (origins || n_origins == 0)), "beam_tally: null beam array");
    OcPut put;
    memset(&put, 0, sizeof(put));
    int64_t cells = 0;
    ST_REQUIRE(beam_off[0] == 0 && beam_off[G] == R, "beam_tally: beam_off runs from %lld to %lld, the beams are %lld", (long long)beam_off[0],
               (long long)beam_off[G], (long long)R);
    for (int g = 0; g < G; g++) {
        const StVoxelGrid& v = grids[g];
        bool fin = v.cell > 0.0f && v.cell <= 3.4028234e38f;
        for (int k = 0; k < 3; k++) {
            fin = fin && fabsf(v.lo[k]) <= 3.4028234e38f;
            ST_REQUIRE(v.dim[k] >= 1 && v.dim[k] <= OC_MAX_DIM, "beam_tally: grid %d has %d cells along axis %d (1 .. %d)", g, (int)v.dim[k], k,
                       OC_MAX_DIM);
            fin = fin && fabsf(v.lo[k] + (float)v.dim[k] * v.cell) <= 3.4028234e38f;
        }
        ST_REQUIRE(fin, "beam_tally: grid %d needs finite corners and a finite cell > 0", g);
        ST_REQUIRE(beam_off[g + 1] >= beam_off[g], "beam_tally: beam_off decreases at grid %d", g);
        OcGrid& d = put.rec[g];
        for (int k = 0; k < 3; k++) { d.lo[k] = v.lo[k]; d.dim[k] = v.dim[k]; }
        d.cell = v.cell;
        d.beam_first = (int32_t)beam_off[g];
        d.cell_base = cells;
        cells += (int64_t)v.dim[0] * v.dim[1] * v.dim[2];
        ST_REQUIRE(cells < (1ll << 31), "beam_tally: the grids of one call have fewer than 2^31 cells (got %lld by grid %d)", (long long)cells, g);
    }
    put.rec[G] = put.rec[G - 1];
    put.rec[G].beam_first = (int32_t)(R < 0x7fffffffll ? R : 0x7fffffffll);
    put.rec[G].cell_base = cells;
    put.count = G + 1;
    StArena arena(ws, ws_bytes);
    OcGrid* table = arena.take<OcGrid>(OC_MAX_GRIDS + 1);
    if (!arena.ok() || !ws) {
        st_set_error("beam_tally: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    (void)hipMemsetAsync(enter, 0, (size_t)cells * sizeof(uint32_t), stream);
    (void)hipMemsetAsync(hit, 0, (size_t)cells * sizeof(uint32_t), stream);
    (void)hipMemsetAsync(behind_out, 0, (size_t)cells * sizeof(uint32_t), stream);
    (void)hipMemsetAsync(path, 0, (size_t)cells * sizeof(uint64_t), stream);
    (void)hipMemsetAsync(counters, 0, 2 * sizeof(uint32_t), stream);
    if (R > 0) {
        hipLaunchKernelGGL(k_oc_put, dim3(1), dim3(128), 0, stream, put, table);
        if (form == 0) form = OC_AUTO_FORM;
        const unsigned blocks = (unsigned)st_div_up(R, OC_BLOCK);
        if (form == 1)
            hipLaunchKernelGGL((k_oc_tally<true>), dim3(blocks), dim3(OC_BLOCK), 0, stream, origins, n_origins, origin_idx, dir, range, R,
                               (const OcGrid*)table, G, max_range, behind ? 1 : 0, enter, hit, behind_out, (unsigned long long*)path, hit_cell,
                               counters);
        else
            hipLaunchKernelGGL((k_oc_tally<false>), dim3(blocks), dim3(OC_BLOCK), 0, stream, origins, n_origins, origin_idx, dir, range, R,
                               (const OcGrid*)table, G, max_range, behind ? 1 : 0, enter, hit, behind_out, (unsigned long long*)path, hit_cell,
                               counters);
    }
    ST_CHECK_LAUNCH();
    return ST_OK;
}
