// st_segment_points_seg: which tube of its cloud's skeleton every point belongs to, batched, with per-tube statistics.
//
// The reference has `skeleton_to_points` (util/queries.py:139-166), a dense sweep that returns distances only; nothing in it says
// which tree and which branch a point belongs to.  This file scores the same pairs and adds what a segmentation needs: a per-cloud
// tube range, an "unassigned" outcome, a strict total order of the candidates, per-tube tallies -- and a grid over the TUBES so
// that a point only meets the tubes around it.
//
// Pair: st_tube.h's (residual = distance to the axis - radius, score = |residual|; tests/segment_oracle.py restates it afresh).
// This file's own rules, on purpose: a zero-length tube (dot(ab, ab) == 0) is the point a with t = 0; a tube with a
// non-finite end point or radius never wins; a point with a non-finite coordinate gets no tube; a NaN score (overflow) never wins.
// Winner: the minimum of (bits of score, tube index).  max_distance >= 0: a best score > max_distance leaves the point unassigned
// (tube -1, residual +inf, vec 0, rad NaN).  tally[3*t ..]: points won, sum of llrintf(score * 2^24), sum of llrintf(residual * 2^24)
// (the scaled value clamped to +-2^62): integer sums, the same in every run and every form.
//
// Form 1, dense: two points per lane (the packed pair), the tubes staged through LDS in tiles, over the union of the tube
//   ranges of the clouds a workgroup's points belong to; a lane takes a tube only inside its own cloud's range.  The loop keeps
//   (score bits, index) only; the winner's pair is evaluated once more at the end (the same operations, the same bits).
// Form 2, grid: per cloud a uniform grid over the boxes of the tubes' axes, each inflated by max(r1, r2, 0); a tube is entered
//   into every cell its box overlaps (count, scan, fill).  A point walks the shells of cells around its own cell (clamped into the
//   grid) and stops once its best score is strictly below a lower bound of every tube it has not met:
//     after shell k every tube listed in a cell within k cells (Chebyshev) of the point's has been met.  A tube not met has, on some
//     axis, a computed cell range disjoint from [i - k, i + k].  The cell coordinate u(v) = floorf((v - lo) / cell), clamped, is
//     monotone in v, and (v - lo) / cell carries two roundings: with at most SG_MAX_DIM = 1024 cells per axis u is within 2^-13 of
//     the exact quotient.  So the box is at least cell * (k - 2^-12) from the point along that axis (clamping only moves a point
//     that lies outside the grid towards the tubes), the axis at least that plus the inflation -- up to the rounding of the box
//     corner, 2^-24 M, M = the largest |coordinate| of a box -- and r(t) <= max(r1, r2) up to 2^-22 M; the computed score differs
//     from the exact one by a few units in the last place of M + |p|.  All of it is covered by
//       bound(k) = k * cell - cell / 16 - 2^-19 * (M + max|p|),
//     and the cell is kept >= 2^-14 M so that the last term stays below cell / 32.
//   A point far from everything, or deep inside a thick tube, finishes with a plain sweep of its cloud's tubes: past SG_MAX_SHELL
//   shells, once the cells read would outnumber twice the cloud's tubes; with max_distance set it stops at the first shell whose
//   bound exceeds max_distance.  A tube met twice is harmless: the minimum is idempotent.  The cell size is chosen on the device -- the mean extent of the boxes, grown until the
//   cell lists and the cell table fit their share of the workspace -- and changes the speed, never the result (st_grid.h's rule).
// Form 0, auto: the grid from SG_AUTO_GRID_M tubes per cloud on (DESIGN.md "Segmentation" has the sweep behind the number).
// Enqueue-only: no allocation, no read-back, no wait.  The first 32 bytes of the workspace hold, after a grid call, four int64:
// points that walked shells, the sum and the maximum of their shell counts, points that ended in the sweep (tools/bench_segment.py).
#include "st_common.h"
#include "st_grid.h"
#include "st_tube.h"

#define SG_BLOCK 256
#define SG_TILE 512
#define SG_NONE 0x7f800001u  // "no score yet": just above the bits of +inf, so neither it nor any NaN score is ever strictly less
#define SG_MAX_DIM 1024
#define SG_MAX_SHELL 4
#define SG_AUTO_GRID_M 20480  // dense and grid cost the same near 19 400 tubes per cloud (profiles/segment_bench.json)
#define SG_PLAN_ROUNDS 96

struct SgCloud {
    float lo[3];
    float cell;
    int dim[3];
    int sweep;          // 1: no usable grid (coordinates beyond 1e18, or the lists did not fit): every point sweeps
    int64_t cell_base;  // the cloud's first cell in the cell table
    int64_t cell_cap, entry_cap;
    float mag;          // M of the bound
    float pad;
};

struct SgStats {
    unsigned long long walked, shells, max_shells, swept;
};

__device__ __forceinline__ bool sg_tube_ok(const float* a, const float* b, const float* r1, const float* r2, int64_t g) {
    return st_finite(a[3 * g]) && st_finite(a[3 * g + 1]) && st_finite(a[3 * g + 2]) && st_finite(b[3 * g]) && st_finite(b[3 * g + 1]) &&
           st_finite(b[3 * g + 2]) && st_finite(r1[g]) && st_finite(r2[g]);
}

// The tube record as every loop here reads it.  A tube with a non-finite value: its radius becomes NaN, and with it every score.
// A zero-length tube (t = 0) without a select in the pair loops: with ab = 0 and the divisor 1 the quotient is +-0, q is a and r is
// r1 -- the score's bits are those of t = 0 (a zero's sign never reaches them; the outputs are formed by sg_finish, which takes
// t = 0 literally).
__device__ __forceinline__ void sg_tube_record(const float* a, const float* b, const float* r1, const float* r2, int64_t g, float4* ta,
                                               float4* tb, float* tab2, int64_t j) {
    const bool ok = sg_tube_ok(a, b, r1, r2, g);
    st_tube_record(a, b, r1, r2, g, ta, tb, tab2, j);
    if (!ok) ta[j].w = __uint_as_float(0x7fc00000u);
    if (tab2[j] == 0.0f) { tb[j].x = 0.0f; tb[j].y = 0.0f; tb[j].z = 0.0f; tab2[j] = 1.0f; }
}

__device__ __forceinline__ long long sg_fix(float v) {  // llrintf(v * 2^24), the scaled value clamped to +-2^62
    const float q = fminf(fmaxf(v * 16777216.0f, -4.611686e18f), 4.611686e18f);
    return llrintf(q);
}

// Outputs of one point from its winner (best < 0: none).  The winner's pair is formed again from the tube's own arrays.
// Returns the tube the point is assigned to (-1: none) and its residual, for the tally.
__device__ __forceinline__ int sg_finish(int64_t i, float px, float py, float pz, int best, float max_distance, const float* a,
                                         const float* b, const float* r1, const float* r2, int32_t* tube, float* residual, float* vec,
                                         float* rad, float* res_out) {
    StPair<float> w;
    w.vx = 0.0f; w.vy = 0.0f; w.vz = 0.0f; w.r = __uint_as_float(0x7fc00000u); w.res = __uint_as_float(0x7f800000u);
    if (best >= 0) {
        float4 A, B;
        float ab2;
        st_tube_record(a, b, r1, r2, best, &A, &B, &ab2, 0);
        const float t = ab2 == 0.0f ? 0.0f : st_tube_t_div(px, py, pz, A, B, ab2);
        const StPair<float> c = st_tube_pair_at(t, px, py, pz, A, B);
        if (max_distance >= 0.0f && fabsf(c.res) > max_distance) best = -1;
        else w = c;
    }
    if (tube) tube[i] = best;
    if (residual) residual[i] = w.res;
    if (vec) { vec[3 * i] = w.vx; vec[3 * i + 1] = w.vy; vec[3 * i + 2] = w.vz; }
    if (rad) rad[i] = w.r;
    *res_out = w.res;
    return best;
}

// The tally of a workgroup's points, summed per tube in LDS first: neighbouring points share their tubes, and a million points on a
// few hundred tubes would otherwise queue on as many addresses (35 ms against 0.2 ms for the whole call, measured).  An open-addressed
// table of SG_TALLY_SLOTS tubes; a point that finds no slot within eight probes adds to global memory itself.  Integer sums: the order
// never shows.  keys [SG_TALLY_SLOTS], cnt_abs [2 * SG_TALLY_SLOTS], sgn [SG_TALLY_SLOTS] are LDS; reached by every thread.
#define SG_TALLY_SLOTS 512
__device__ __forceinline__ void sg_tally_add(int won, float res, int* keys, unsigned long long* cnt_abs, unsigned long long* sgn,
                                             unsigned long long* tally) {
    if (won < 0) return;
    const unsigned long long fa = (unsigned long long)sg_fix(fabsf(res)), fs = (unsigned long long)sg_fix(res);
    unsigned slot = ((unsigned)won * 2654435761u) >> 23;  // 9 bits
    for (int probe = 0; probe < 8; probe++, slot = (slot + 1u) & (SG_TALLY_SLOTS - 1)) {
        const int prev = atomicCAS(&keys[slot], -1, won);
        if (prev == -1 || prev == won) {
            atomicAdd(&cnt_abs[2 * slot], 1ull);
            atomicAdd(&cnt_abs[2 * slot + 1], fa);
            atomicAdd(&sgn[slot], fs);
            return;
        }
    }
    atomicAdd(&tally[3 * (int64_t)won], 1ull);
    atomicAdd(&tally[3 * (int64_t)won + 1], fa);
    atomicAdd(&tally[3 * (int64_t)won + 2], fs);
}
__device__ __forceinline__ void sg_tally_clear(int* keys, unsigned long long* cnt_abs, unsigned long long* sgn) {
    for (int j = threadIdx.x; j < SG_TALLY_SLOTS; j += blockDim.x) { keys[j] = -1; cnt_abs[2 * j] = 0ull; cnt_abs[2 * j + 1] = 0ull; sgn[j] = 0ull; }
}
__device__ __forceinline__ void sg_tally_flush(const int* keys, const unsigned long long* cnt_abs, const unsigned long long* sgn,
                                               unsigned long long* tally) {
    for (int j = threadIdx.x; j < SG_TALLY_SLOTS; j += blockDim.x) {
        const int t = keys[j];
        if (t < 0) continue;
        atomicAdd(&tally[3 * (int64_t)t], cnt_abs[2 * j]);
        atomicAdd(&tally[3 * (int64_t)t + 1], cnt_abs[2 * j + 1]);
        atomicAdd(&tally[3 * (int64_t)t + 2], sgn[j]);
    }
}

// ------------------------------------------------------------------------------------ form 1: dense ---
// BATCH = false: one cloud, every tube is in range.
template <bool BATCH>
__global__ void __launch_bounds__(SG_BLOCK) k_sg_dense(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ pt_seg_off,
                                                       const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ r1, const float* __restrict__ r2, int64_t m,
                                                       const int32_t* __restrict__ tube_seg_off, int nseg, float max_distance,
                                                       int32_t* tube, float* residual, float* vec, float* rad, int64_t* tally) {
    // per tube: (a.xyz, r1), (ab.xyz, r2), ab.ab -- three LDS reads per tube, the same address in every lane (broadcast)
    __shared__ float4 ta[SG_TILE], tb[SG_TILE];
    __shared__ float tab2[SG_TILE];
    const int64_t first = (int64_t)blockIdx.x * (2 * SG_BLOCK);
    const int64_t last = first + 2 * SG_BLOCK < n ? first + 2 * SG_BLOCK - 1 : n - 1;
    const int64_t i0 = first + 2 * (int64_t)threadIdx.x, i1 = i0 + 1;
    const bool live0 = i0 < n, live1 = i1 < n;
    // the tubes this workgroup streams: from the first tube of its first point's cloud to the last tube of its last point's
    int64_t t_begin = 0, t_end = m;
    int lo0 = 0, lo1 = 0;
    unsigned cnt0 = (unsigned)m, cnt1 = (unsigned)m;  // the lane's own ranges: tube g counts iff (unsigned)(g - lo) < cnt
    if (BATCH) {
        t_begin = tube_seg_off[st_seg_find(pt_seg_off, nseg, first)];
        t_end = tube_seg_off[st_seg_find(pt_seg_off, nseg, last) + 1];
        const int s0 = st_seg_find(pt_seg_off, nseg, live0 ? i0 : last), s1 = st_seg_find(pt_seg_off, nseg, live1 ? i1 : last);
        lo0 = tube_seg_off[s0]; cnt0 = (unsigned)(tube_seg_off[s0 + 1] - lo0);
        lo1 = tube_seg_off[s1]; cnt1 = (unsigned)(tube_seg_off[s1 + 1] - lo1);
    }
    const st_f2 px = {live0 ? pts[3 * i0] : 0.0f, live1 ? pts[3 * i1] : 0.0f};
    const st_f2 py = {live0 ? pts[3 * i0 + 1] : 0.0f, live1 ? pts[3 * i1 + 1] : 0.0f};
    const st_f2 pz = {live0 ? pts[3 * i0 + 2] : 0.0f, live1 ? pts[3 * i1 + 2] : 0.0f};
    unsigned key0 = SG_NONE, key1 = SG_NONE;
    int best0 = -1, best1 = -1;
    st_tube_sweep<SG_BLOCK, SG_TILE>(
        t_begin, t_end, live0, [&](int64_t g, int j) { sg_tube_record(a, b, r1, r2, g, ta, tb, tab2, j); },
        [&](int j, int g) {
            const StPair<st_f2> c = st_tube_pair(px, py, pz, ta[j], tb[j], tab2[j]);
            const unsigned k0 = __float_as_uint(fabsf(c.res.x)), k1 = __float_as_uint(fabsf(c.res.y));
            if (k0 < key0 && (!BATCH || (unsigned)(g - lo0) < cnt0)) { key0 = k0; best0 = g; }  // score >= 0: the bits order like the values
            if (k1 < key1 && (!BATCH || (unsigned)(g - lo1) < cnt1)) { key1 = k1; best1 = g; }
        });
    int won0 = -1, won1 = -1;
    float res0 = 0.0f, res1 = 0.0f;
    if (live0) {
        if (!(st_finite(px.x) && st_finite(py.x) && st_finite(pz.x))) best0 = -1;
        won0 = sg_finish(i0, px.x, py.x, pz.x, best0, max_distance, a, b, r1, r2, tube, residual, vec, rad, &res0);
    }
    if (live1) {
        if (!(st_finite(px.y) && st_finite(py.y) && st_finite(pz.y))) best1 = -1;
        won1 = sg_finish(i1, px.y, py.y, pz.y, best1, max_distance, a, b, r1, r2, tube, residual, vec, rad, &res1);
    }
    if (tally == nullptr) return;  // (the same in every lane)
    // the tile arrays are done with: the tally's table lives in them (tab2: 512 keys, ta: 1024 sums, tb: 512 sums)
    int* keys = (int*)tab2;
    unsigned long long *cnt_abs = (unsigned long long*)ta, *sgn = (unsigned long long*)tb;
    __syncthreads();
    sg_tally_clear(keys, cnt_abs, sgn);
    __syncthreads();
    sg_tally_add(won0, res0, keys, cnt_abs, sgn, (unsigned long long*)tally);
    sg_tally_add(won1, res1, keys, cnt_abs, sgn, (unsigned long long*)tally);
    __syncthreads();
    sg_tally_flush(keys, cnt_abs, sgn, (unsigned long long*)tally);
}

// ------------------------------------------------------------------------------------- form 2: grid ---
// the box of tube g's axis inflated by max(r1, r2, 0); false for a tube that never wins (it enters no cell)
__device__ __forceinline__ bool sg_box(const float* a, const float* b, const float* r1, const float* r2, int64_t g, float* lo, float* hi) {
    if (!sg_tube_ok(a, b, r1, r2, g)) return false;
    const float infl = fmaxf(fmaxf(r1[g], r2[g]), 0.0f);
    for (int k = 0; k < 3; k++) {
        lo[k] = fminf(a[3 * g + k], b[3 * g + k]) - infl;
        hi[k] = fmaxf(a[3 * g + k], b[3 * g + k]) + infl;
    }
    return true;
}
// cell of coordinate v along one axis, clamped AS A FLOAT (a point far outside the box must not reach the integer conversion);
// monotone in v
__device__ __forceinline__ int sg_axis(float v, float lo, float cell, int dim) {
    float c = floorf((v - lo) / cell);
    c = fminf(fmaxf(c, 0.0f), (float)(dim - 1));
    return (int)c;
}

// One workgroup per cloud: the box of the tubes' boxes, the cell size and the grid's shape.
__global__ void __launch_bounds__(SG_BLOCK) k_sg_plan(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                      const int32_t* tube_seg_off, int nseg, int cells_per_tube, int entries_per_tube,
                                                      SgCloud* clouds, SgStats* stats) {
    __shared__ float s_lo[3][SG_BLOCK], s_hi[3][SG_BLOCK], s_ext[SG_BLOCK], s_mag[SG_BLOCK];
    __shared__ unsigned s_cnt[SG_BLOCK];
    __shared__ unsigned long long s_sum[SG_BLOCK];
    __shared__ float g_lo[3], g_hi[3], g_cell;
    __shared__ int g_dim[3], g_state;  // 0: try this cell size, 1: it fits, 2: give up (sweep)
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = tube_seg_off != nullptr && nseg > 1 ? tube_seg_off[s] : 0;
    const int64_t t1 = tube_seg_off != nullptr && nseg > 1 ? tube_seg_off[s + 1] : m;
    const int64_t cell_base = (int64_t)cells_per_tube * t0 + 64 * (int64_t)s;
    const int64_t cell_cap = (int64_t)cells_per_tube * (t1 - t0) + 64, entry_cap = (int64_t)entries_per_tube * (t1 - t0) + 64;
    if (s == 0 && tid == 0) { stats->walked = 0ull; stats->shells = 0ull; stats->max_shells = 0ull; stats->swept = 0ull; }
    const float big = 3.4028234e38f;
    float lo[3] = {big, big, big}, hi[3] = {-big, -big, -big}, ext = 0.0f, mag = 0.0f;
    unsigned cnt = 0u;
    for (int64_t g = t0 + tid; g < t1; g += SG_BLOCK) {
        float bl[3], bh[3];
        if (!sg_box(a, b, r1, r2, g, bl, bh)) continue;
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], bl[k]);
            hi[k] = fmaxf(hi[k], bh[k]);
            mag = fmaxf(mag, fmaxf(fabsf(bl[k]), fabsf(bh[k])));
        }
        ext += fmaxf(fmaxf(bh[0] - bl[0], bh[1] - bl[1]), bh[2] - bl[2]);
        cnt++;
    }
    for (int k = 0; k < 3; k++) { s_lo[k][tid] = lo[k]; s_hi[k][tid] = hi[k]; }
    s_ext[tid] = ext; s_mag[tid] = mag; s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        float e = 0.0f, mg = 0.0f;
        unsigned c = 0u;
        for (int k = 0; k < 3; k++) { g_lo[k] = big; g_hi[k] = -big; }
        for (int j = 0; j < SG_BLOCK; j++) {
            for (int k = 0; k < 3; k++) { g_lo[k] = fminf(g_lo[k], s_lo[k][j]); g_hi[k] = fmaxf(g_hi[k], s_hi[k][j]); }
            e += s_ext[j]; mg = fmaxf(mg, s_mag[j]); c += s_cnt[j];
        }
        s_mag[0] = mg;
        g_state = 0;
        if (c == 0u) {  // no tube that can win: one empty cell
            for (int k = 0; k < 3; k++) { g_lo[k] = 0.0f; g_hi[k] = 0.0f; }
            g_cell = 1.0f;
        } else if (!(mg <= 1.0e18f)) {
            g_state = 2;
            g_cell = 1.0f;
        } else {
            g_cell = fmaxf(fmaxf(e / (float)c, mg * 6.1035156e-5f), 1.0e-6f);  // the mean extent; >= 2^-14 M
        }
    }
    __syncthreads();
    for (int round = 0; round < SG_PLAN_ROUNDS; round++) {
        if (g_state != 0) break;  // (the same in every lane: read after a barrier, written before the next)
        const float cell = g_cell;
        if (tid < 3) {
            float d = floorf((g_hi[tid] - g_lo[tid]) / cell) + 1.0f;
            g_dim[tid] = (int)fminf(fmaxf(d, 1.0f), (float)SG_MAX_DIM);
        }
        __syncthreads();
        unsigned long long sum = 0ull;  // an upper bound of the entries this cell size makes
        for (int64_t g = t0 + tid; g < t1; g += SG_BLOCK) {
            float bl[3], bh[3];
            if (!sg_box(a, b, r1, r2, g, bl, bh)) continue;
            unsigned long long p = 1ull;
            for (int k = 0; k < 3; k++) p *= (unsigned long long)fminf((float)g_dim[k], floorf((bh[k] - bl[k]) / cell) + 3.0f);
            sum += p;
        }
        s_sum[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            unsigned long long total = 0ull;
            for (int j = 0; j < SG_BLOCK; j++) total += s_sum[j];
            const bool dims_ok = (g_hi[0] - g_lo[0]) / cell < (float)SG_MAX_DIM && (g_hi[1] - g_lo[1]) / cell < (float)SG_MAX_DIM &&
                                 (g_hi[2] - g_lo[2]) / cell < (float)SG_MAX_DIM;
            const int64_t ncell = (int64_t)g_dim[0] * g_dim[1] * g_dim[2];
            if (dims_ok && ncell <= cell_cap && total <= (unsigned long long)entry_cap) g_state = 1;
            else if (round == SG_PLAN_ROUNDS - 1) g_state = 2;
            else g_cell = cell * 1.25f;
        }
        __syncthreads();
    }
    if (tid == 0) {
        SgCloud c;
        const bool sweep = g_state != 1;
        for (int k = 0; k < 3; k++) { c.lo[k] = g_lo[k]; c.dim[k] = sweep ? 1 : g_dim[k]; }
        c.cell = g_cell;
        c.sweep = sweep ? 1 : 0;
        c.cell_base = cell_base;
        c.cell_cap = cell_cap;
        c.entry_cap = entry_cap;
        c.mag = s_mag[0];
        c.pad = 0.0f;
        clouds[s] = c;
    }
}

// FILL = false: count the tubes of every cell; FILL = true: write them behind the cell's start.  A lane per tube.
template <bool FILL>
__global__ void __launch_bounds__(SG_BLOCK) k_sg_bin(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                     const int32_t* tube_seg_off, int nseg, const SgCloud* clouds, uint32_t* cell_cnt,
                                                     const uint32_t* cell_start, uint32_t* entries, int64_t entry_total) {
    const int64_t g = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    if (g >= m) return;
    float bl[3], bh[3];
    if (!sg_box(a, b, r1, r2, g, bl, bh)) return;
    const SgCloud* c = clouds + st_seg_find(tube_seg_off, nseg, g);
    if (c->sweep) return;
    const int x0 = sg_axis(bl[0], c->lo[0], c->cell, c->dim[0]), x1 = sg_axis(bh[0], c->lo[0], c->cell, c->dim[0]);
    const int y0 = sg_axis(bl[1], c->lo[1], c->cell, c->dim[1]), y1 = sg_axis(bh[1], c->lo[1], c->cell, c->dim[1]);
    const int z0 = sg_axis(bl[2], c->lo[2], c->cell, c->dim[2]), z1 = sg_axis(bh[2], c->lo[2], c->cell, c->dim[2]);
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

// offer tube g to a point
__device__ __forceinline__ void sg_offer(float px, float py, float pz, int g, const float4* ta, const float4* tb, const float* tab2,
                                         unsigned* key, int* best) {
    const unsigned k = __float_as_uint(fabsf(st_tube_pair(px, py, pz, ta[g], tb[g], tab2[g]).res));
    if (k < *key || (k == *key && g < *best)) { *key = k; *best = g; }
}

// the tubes as the pair reads them, for the grid form's gathers
__global__ void __launch_bounds__(SG_BLOCK) k_sg_pack(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                      float4* ta, float4* tb, float* tab2) {
    const int64_t g = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    if (g >= m) return;
    sg_tube_record(a, b, r1, r2, g, ta, tb, tab2, g);
}

__global__ void __launch_bounds__(SG_BLOCK) k_sg_query(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ pt_seg_off,
                                                       int nseg, const SgCloud* __restrict__ clouds, const uint32_t* __restrict__ cell_start,
                                                       const uint32_t* __restrict__ entries, int64_t entry_total,
                                                       const float4* __restrict__ ta, const float4* __restrict__ tb,
                                                       const float* __restrict__ tab2, const float* a, const float* b, const float* r1,
                                                       const float* r2, int64_t m, const int32_t* __restrict__ tube_seg_off,
                                                       float max_distance, int32_t* tube, float* residual, float* vec, float* rad,
                                                       int64_t* tally, SgStats* stats) {
    __shared__ unsigned s_walked, s_shells, s_max, s_swept;
    __shared__ int keys[SG_TALLY_SLOTS];
    __shared__ unsigned long long cnt_abs[2 * SG_TALLY_SLOTS], sgn[SG_TALLY_SLOTS];
    if (threadIdx.x == 0) { s_walked = 0u; s_shells = 0u; s_max = 0u; s_swept = 0u; }
    if (tally) sg_tally_clear(keys, cnt_abs, sgn);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    if (i < n) {
        const int s = st_seg_find(pt_seg_off, nseg, i);
        const SgCloud* c = clouds + s;
        const int t0 = tube_seg_off != nullptr && nseg > 1 ? tube_seg_off[s] : 0;
        const int t1 = tube_seg_off != nullptr && nseg > 1 ? tube_seg_off[s + 1] : (int)m;
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        unsigned key = SG_NONE;
        int best = -1;
        if (st_finite(px) && st_finite(py) && st_finite(pz)) {
            bool sweep = c->sweep != 0;
            if (!sweep) {
                const int dx = c->dim[0], dy = c->dim[1], dz = c->dim[2];
                const float cell = c->cell;
                const int ix = sg_axis(px, c->lo[0], cell, dx), iy = sg_axis(py, c->lo[1], cell, dy), iz = sg_axis(pz, c->lo[2], cell, dz);
                const float slack = cell * 0.0625f + 1.9073486e-6f * (c->mag + fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)));
                int k = 0;
                for (;; k++) {
                    const int x0 = st_max(ix - k, 0), x1 = st_min(ix + k, dx - 1), y0 = st_max(iy - k, 0), y1 = st_min(iy + k, dy - 1);
                    const int z0 = st_max(iz - k, 0), z1 = st_min(iz + k, dz - 1);
                    for (int x = x0; x <= x1; x++)
                        for (int y = y0; y <= y1; y++) {
                            const bool face = x == ix - k || x == ix + k || y == iy - k || y == iy + k;  // the whole z-run is new
                            const int64_t row = c->cell_base + ((int64_t)x * dy + y) * dz;
                            for (int z = z0; z <= z1; z++) {
                                if (!face && z != iz - k && z != iz + k) continue;  // inside the cube: met in an earlier shell
                                uint32_t u = cell_start[row + z], e = cell_start[row + z + 1];
                                if ((int64_t)e > entry_total) e = (uint32_t)entry_total;
                                for (; u < e; u++) sg_offer(px, py, pz, (int)entries[u], ta, tb, tab2, &key, &best);
                            }
                        }
                    if (ix - k <= 0 && ix + k >= dx - 1 && iy - k <= 0 && iy + k >= dy - 1 && iz - k <= 0 && iz + k >= dz - 1) break;
                    const float bound = (float)k * cell - slack;  // everything not met scores at least this
                    if (__uint_as_float(key) < bound || (max_distance >= 0.0f && max_distance < bound)) break;  // (SG_NONE is a NaN)
                    // the next shell would bring the cells read to (2k + 3)^3: beyond twice the cloud's tubes the plain sweep is cheaper
                    const int64_t w = 2 * (int64_t)k + 3;
                    if (k >= SG_MAX_SHELL && w * w * w > 2 * (int64_t)(t1 - t0)) { sweep = true; break; }
                }
                atomicAdd(&s_walked, 1u);
                atomicAdd(&s_shells, (unsigned)(k + 1));
                atomicMax(&s_max, (unsigned)(k + 1));
            }
            if (sweep) {
                for (int g = t0; g < t1; g++) sg_offer(px, py, pz, g, ta, tb, tab2, &key, &best);
                atomicAdd(&s_swept, 1u);
            }
        }
        float res = 0.0f;
        const int won = sg_finish(i, px, py, pz, best, max_distance, a, b, r1, r2, tube, residual, vec, rad, &res);
        if (tally) sg_tally_add(won, res, keys, cnt_abs, sgn, (unsigned long long*)tally);
    }
    __syncthreads();
    if (tally) sg_tally_flush(keys, cnt_abs, sgn, (unsigned long long*)tally);
    if (threadIdx.x == 0) {
        if (s_walked) { atomicAdd(&stats->walked, (unsigned long long)s_walked); atomicAdd(&stats->shells, (unsigned long long)s_shells); }
        if (s_max) atomicMax(&stats->max_shells, (unsigned long long)s_max);
        if (s_swept) atomicAdd(&stats->swept, (unsigned long long)s_swept);
    }
}

// --------------------------------------------------------------------------------------- host ---
struct SgLayout {
    SgStats* stats;
    SgCloud* clouds;
    float4 *ta, *tb;
    float* tab2;
    uint32_t *cell_cnt, *cell_start, *entries;
    char* sws;
    int64_t cells, entry_total, sws_bytes;
    int cells_per_tube, entries_per_tube;
};

static void sg_layout(StArena& a, int64_t m, int nseg, SgLayout* L) {
    const int64_t mm = m > 0 ? m : 1;
    // every cloud's share of the tables is a multiple of its tubes: smaller multiples for huge skeletons keep the totals below 2^31
    L->cells_per_tube = (int)st_min64(8, (1ll << 28) / mm > 0 ? (1ll << 28) / mm : 1);
    L->entries_per_tube = (int)st_min64(32, (1ll << 30) / mm > 0 ? (1ll << 30) / mm : 1);
    L->cells = (int64_t)L->cells_per_tube * m + 64 * (int64_t)nseg;
    L->entry_total = (int64_t)L->entries_per_tube * m + 64 * (int64_t)nseg;
    L->stats = a.take<SgStats>(1);
    L->clouds = a.take<SgCloud>(ST_MAX_SEG);
    L->ta = a.take<float4>(m);
    L->tb = a.take<float4>(m);
    L->tab2 = a.take<float>(m);
    L->cell_cnt = a.take<uint32_t>(L->cells + 1);
    L->cell_start = a.take<uint32_t>(L->cells + 1);
    L->entries = a.take<uint32_t>(L->entry_total);
    L->sws_bytes = st_scan_ws_bytes(L->cells + 1);
    L->sws = a.take<char>(L->sws_bytes);
}

static bool sg_sizes_ok(int64_t n, int64_t m, int nseg) {
    return n >= 0 && m >= 0 && n < (1ll << 31) && m < (1ll << 31) && nseg >= 1 && nseg <= ST_MAX_SEG;
}

extern "C" int64_t st_segment_workspace_bytes(int64_t n, int64_t m, int nseg) {
    if (!sg_sizes_ok(n, m, nseg)) return -1;
    StArena a(nullptr, 0);
    SgLayout L;
    sg_layout(a, m, nseg, &L);
    return a.used;
}

// pts [n,3]; a, b [m,3], r1, r2 [m]: the tubes; pt_seg_off, tube_seg_off [nseg + 1] (null: one cloud); outputs nullable.
extern "C" int st_segment_points_seg(const float* pts, int64_t n, const int32_t* pt_seg_off, const float* a, const float* b,
                                     const float* r1, const float* r2, int64_t m, const int32_t* tube_seg_off, int nseg,
                                     float max_distance, int form, int32_t* tube, float* residual, float* vec, float* rad, int64_t* tally,
                                     void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n >= 0 && n < (1ll << 31), "segment_points: 0 <= points < 2^31 (got %lld)", (long long)n);
    ST_REQUIRE(m >= 0 && m < (1ll << 31), "segment_points: 0 <= tubes < 2^31 (got %lld)", (long long)m);
    ST_REQUIRE(nseg >= 1 && nseg <= ST_MAX_SEG, "segment_points: 1 <= clouds per batch <= %d (got %d)", ST_MAX_SEG, nseg);
    ST_REQUIRE(nseg == 1 || (pt_seg_off && tube_seg_off), "segment_points: %d clouds need the offsets of their points and of their tubes", nseg);
    ST_REQUIRE(max_distance == max_distance, "segment_points: max_distance is NaN (negative means unbounded)");
    ST_REQUIRE(form >= 0 && form <= 2, "segment_points: form must be 0 (auto), 1 (dense) or 2 (grid), got %d", form);
    StArena arena(ws, ws_bytes);
    SgLayout L;
    sg_layout(arena, m, nseg, &L);
    if (!arena.ok() || !ws) {
        st_set_error("segment_points: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (nseg == 1) { pt_seg_off = nullptr; tube_seg_off = nullptr; }
    if (tally && m > 0) (void)hipMemsetAsync(tally, 0, (size_t)(3 * m) * sizeof(int64_t), stream);
    if (n == 0) { ST_CHECK_LAUNCH(); return ST_OK; }
    if (form == 0) form = m / nseg >= SG_AUTO_GRID_M ? 2 : 1;
    if (m == 0) form = 1;  // nothing to bin: the dense loop over no tubes leaves every point unassigned
    if (form == 1) {
        if (nseg > 1)
            hipLaunchKernelGGL((k_sg_dense<true>), dim3((unsigned)st_div_up(n, 2 * SG_BLOCK)), dim3(SG_BLOCK), 0, stream, pts, n, pt_seg_off,
                               a, b, r1, r2, m, tube_seg_off, nseg, max_distance, tube, residual, vec, rad, tally);
        else
            hipLaunchKernelGGL((k_sg_dense<false>), dim3((unsigned)st_div_up(n, 2 * SG_BLOCK)), dim3(SG_BLOCK), 0, stream, pts, n, pt_seg_off,
                               a, b, r1, r2, m, tube_seg_off, nseg, max_distance, tube, residual, vec, rad, tally);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    const unsigned mb = (unsigned)st_div_up(m, SG_BLOCK);
    hipLaunchKernelGGL(k_sg_plan, dim3((unsigned)nseg), dim3(SG_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, nseg, L.cells_per_tube,
                       L.entries_per_tube, L.clouds, L.stats);
    hipLaunchKernelGGL(k_sg_pack, dim3(mb), dim3(SG_BLOCK), 0, stream, a, b, r1, r2, m, L.ta, L.tb, L.tab2);
    (void)hipMemsetAsync(L.cell_cnt, 0, (size_t)(L.cells + 1) * sizeof(uint32_t), stream);
    hipLaunchKernelGGL((k_sg_bin<false>), dim3(mb), dim3(SG_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, nseg,
                       (const SgCloud*)L.clouds, L.cell_cnt, (const uint32_t*)nullptr, (uint32_t*)nullptr, L.entry_total);
    ST_TRY(st_exclusive_scan_u32(L.cell_cnt, L.cell_start, L.cells + 1, nullptr, L.sws, L.sws_bytes, stream));
    (void)hipMemsetAsync(L.cell_cnt, 0, (size_t)(L.cells + 1) * sizeof(uint32_t), stream);
    hipLaunchKernelGGL((k_sg_bin<true>), dim3(mb), dim3(SG_BLOCK), 0, stream, a, b, r1, r2, m, tube_seg_off, nseg,
                       (const SgCloud*)L.clouds, L.cell_cnt, (const uint32_t*)L.cell_start, L.entries, L.entry_total);
    hipLaunchKernelGGL(k_sg_query, dim3((unsigned)st_div_up(n, SG_BLOCK)), dim3(SG_BLOCK), 0, stream, pts, n, pt_seg_off, nseg,
                       (const SgCloud*)L.clouds, (const uint32_t*)L.cell_start, (const uint32_t*)L.entries, L.entry_total,
                       (const float4*)L.ta, (const float4*)L.tb, (const float*)L.tab2, a, b, r1, r2, m, tube_seg_off, max_distance, tube,
                       residual, vec, rad, tally, L.stats);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
