// st_tree_tally: what every tree of a segmented cloud occupies -- its box, its points per class and the distinct cells of its
// crown in plan and, by height layer, in volume.  Integers and extrema only: the same bits in every run.
//
// The reference measures nothing (BranchSkeleton.length / TreeSkeleton.length are its only quantities); smart_tree_amd/inventory.py
// turns these tallies and the skeleton into height, crown extent, crown area and crown volume per tree.
//
// The contract (tests/inventory_oracle.py restates it on its own, on purpose).
// Who takes part: point i with three finite coordinates, 0 <= tree[i] < n_trees and (cls == NULL or cls[i] < n_classes).
// box [6*T] float32: min x, y, z then max x, y, z over the tree's points, compared as st_f2ord orders floats (-0 below +0);
//   (+inf x3, -inf x3) without points.  counts [T*C] int64 (C = n_classes, 1 with cls == NULL): points per tree and class.
// Cell of a point, in its tree's box (float32, no contraction): i_k = (int)min(max(floorf((p_k - min_k) / cell), 0), 16383).
//   up in 0..2 is the vertical axis, h0 < h1 the other two; layer = min(i_up, layers - 1).
// area_cells [T] int64: distinct (i_h0, i_h1) of the tree.  profile [T*layers] int64: distinct (i_h0, i_h1, i_up) per layer (the
//   triples above the last layer stay distinct and count there).
//
// Two dependent passes over the points (the cells need the boxes), then one lane per box value.
// k_tt_box: a thread keeps the extrema and the count of the run of equal trees it reads (TT_TILES points) in registers and hands
//   each run to a per-workgroup LDS table (TT_TREES trees, TT_COUNTS (tree, class) pairs, open addressing, TT_PROBES probes); a run
//   that finds no slot goes to global memory itself; every occupied slot is flushed once.  One global atomic per point and axis on
//   a handful of addresses is the pattern segment.hip's tally measured 250 times slower.
// k_tt_cells: up to two 64-bit keys per point -- family (1 bit: plan 0, volume 1) | tree (21) | i_up (14, 0 in a plan key) | i_h1 (14)
//   | i_h0 (14) -- into one open-addressing set in the workspace: home slot st_hash64(key), then the next slot, wrapping.  The walk
//   visits every slot and the set is at most half full (2n keys in >= 4n slots), so it always meets the key or an empty slot.
//   (st_hash_next keeps a key inside one eighth of the table: a set of 16 slots would have two for it.)
//   tree <= 2^21 - 2, so no key is the empty marker (all ones).  A slot is read first and CAS'd only when empty; a key
//   never changes once written.  The lane whose CAS installs a key adds 1 to that key's counter: exactly one lane per distinct key,
//   whatever the order.  Most points repeat a cell: a workgroup first offers a key to an LDS set of TT_SET slots
//   and only the lane that installs it there (or finds no slot in TT_PROBES probes) goes to global memory.
// Enqueue-only: no allocation, no read-back, no wait.
#include "st_common.h"
#include "st_tube.h"

#define TT_BLOCK 256
#define TT_TILES 8      // points per workgroup = TT_TILES * TT_BLOCK, strided by TT_BLOCK: a thread's run is TT_TILES points
#define TT_TREES 64     // LDS box table: 64 x (key + 6 words) = 1.75 KB
#define TT_COUNTS 128   // LDS count table: 128 x (key + count) = 1 KB
#define TT_PROBES 4
#define TT_SET 2048     // LDS key set of the cell pass: 16 KB, one slot per point of the workgroup
#define TT_MAX_INDEX 16383.0f
#define TT_MAX_TREES (1ll << 21)
#define TT_ORD_POS_INF 0xff800000u  // st_f2ord(+inf)
#define TT_ORD_NEG_INF 0x007fffffu  // st_f2ord(-inf)

// Does point i take part?  Its tree, class and coordinates when it does.
__device__ __forceinline__ bool tt_point(const float* __restrict__ pts, const int32_t* __restrict__ tree, const uint8_t* __restrict__ cls,
                                         int n_classes, int64_t n_trees, int64_t i, int* t, int* c, float* p) {
    const int tr = tree[i];
    if (tr < 0 || (int64_t)tr >= n_trees) return false;
    const int cl = cls ? (int)cls[i] : 0;
    if (cl >= n_classes) return false;
    p[0] = pts[3 * i]; p[1] = pts[3 * i + 1]; p[2] = pts[3 * i + 2];
    if (!(st_finite(p[0]) && st_finite(p[1]) && st_finite(p[2]))) return false;
    *t = tr;
    *c = cl;
    return true;
}

__global__ void __launch_bounds__(TT_BLOCK) k_tt_init(unsigned* boxord, int64_t n_trees) {
    const int64_t g = (int64_t)blockIdx.x * TT_BLOCK + threadIdx.x;
    if (g >= 6 * n_trees) return;
    boxord[g] = (g % 6) < 3 ? TT_ORD_POS_INF : TT_ORD_NEG_INF;
}

__global__ void __launch_bounds__(TT_BLOCK) k_tt_box_out(const unsigned* __restrict__ boxord, int64_t n_trees, float* box) {
    const int64_t g = (int64_t)blockIdx.x * TT_BLOCK + threadIdx.x;
    if (g >= 6 * n_trees) return;
    box[g] = st_ord2f(boxord[g]);
}

// One run of a thread (tree t, ordered extrema lo / hi) into the workgroup's table, or into global memory when it holds no slot.
__device__ __forceinline__ void tt_box_run(int* keys, unsigned* ext, unsigned* boxord, int t, const unsigned* lo, const unsigned* hi) {
    unsigned slot = ((unsigned)t * 2654435761u) >> 26;  // 6 bits
    for (int probe = 0; probe < TT_PROBES; probe++, slot = (slot + 1u) & (TT_TREES - 1)) {
        const int prev = atomicCAS(&keys[slot], -1, t);
        if (prev == -1 || prev == t) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                atomicMin(&ext[k * TT_TREES + slot], lo[k]);
                atomicMax(&ext[(3 + k) * TT_TREES + slot], hi[k]);
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {  // more trees among this workgroup's points than the table holds
        atomicMin(&boxord[6 * (int64_t)t + k], lo[k]);
        atomicMax(&boxord[6 * (int64_t)t + 3 + k], hi[k]);
    }
}

// pair = tree * n_classes + class: the position in counts.
__device__ __forceinline__ void tt_count_run(unsigned long long* keys, unsigned* sums, unsigned long long* counts,
                                             unsigned long long pair, unsigned run) {
    unsigned slot = (unsigned)(st_hash64(pair) >> 57);  // 7 bits
    for (int probe = 0; probe < TT_PROBES; probe++, slot = (slot + 1u) & (TT_COUNTS - 1)) {
        const unsigned long long prev = atomicCAS(&keys[slot], (unsigned long long)ST_EMPTY_KEY, pair);
        if (prev == ST_EMPTY_KEY || prev == pair) {
            atomicAdd(&sums[slot], run);
            return;
        }
    }
    atomicAdd(&counts[pair], (unsigned long long)run);
}

// ext [6 * TT_TREES] is value-major (the lanes of a wave-instruction spread over the slots), as fit.hip's sums.
__global__ void __launch_bounds__(TT_BLOCK) k_tt_box(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ tree,
                                                     const uint8_t* __restrict__ cls, int n_classes, int64_t n_trees, unsigned* boxord,
                                                     unsigned long long* counts) {
    __shared__ int keys[TT_TREES];
    __shared__ unsigned ext[6 * TT_TREES];
    __shared__ unsigned long long pair_keys[TT_COUNTS];
    __shared__ unsigned pair_sums[TT_COUNTS];
    for (int j = threadIdx.x; j < TT_TREES; j += TT_BLOCK) keys[j] = -1;
    for (int j = threadIdx.x; j < 6 * TT_TREES; j += TT_BLOCK) ext[j] = j < 3 * TT_TREES ? TT_ORD_POS_INF : TT_ORD_NEG_INF;
    for (int j = threadIdx.x; j < TT_COUNTS; j += TT_BLOCK) { pair_keys[j] = ST_EMPTY_KEY; pair_sums[j] = 0u; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (TT_TILES * TT_BLOCK);
    int run_t = -1;
    unsigned long long run_pair = ST_EMPTY_KEY;
    unsigned run = 0u;
    unsigned lo[3] = {TT_ORD_POS_INF, TT_ORD_POS_INF, TT_ORD_POS_INF}, hi[3] = {TT_ORD_NEG_INF, TT_ORD_NEG_INF, TT_ORD_NEG_INF};
    for (int tile = 0; tile < TT_TILES; tile++) {
        const int64_t i = base + (int64_t)tile * TT_BLOCK + threadIdx.x;
        if (i >= n) break;
        int t, c;
        float p[3];
        if (!tt_point(pts, tree, cls, n_classes, n_trees, i, &t, &c, p)) continue;
        if (t != run_t) {
            if (run_t >= 0) tt_box_run(keys, ext, boxord, run_t, lo, hi);
            run_t = t;
#pragma unroll
            for (int k = 0; k < 3; k++) { lo[k] = TT_ORD_POS_INF; hi[k] = TT_ORD_NEG_INF; }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned o = st_f2ord(p[k]);
            lo[k] = st_min(lo[k], o);
            hi[k] = st_max(hi[k], o);
        }
        if (counts) {
            const unsigned long long pair = (unsigned long long)t * (unsigned)n_classes + (unsigned)c;
            if (pair != run_pair) {
                if (run_pair != ST_EMPTY_KEY) tt_count_run(pair_keys, pair_sums, counts, run_pair, run);
                run_pair = pair;
                run = 0u;
            }
            run++;
        }
    }
    if (run_t >= 0) tt_box_run(keys, ext, boxord, run_t, lo, hi);
    if (run_pair != ST_EMPTY_KEY) tt_count_run(pair_keys, pair_sums, counts, run_pair, run);
    __syncthreads();
    for (int j = threadIdx.x; j < TT_TREES; j += TT_BLOCK) {
        const int t = keys[j];
        if (t < 0) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&boxord[6 * (int64_t)t + k], ext[k * TT_TREES + j]);
            atomicMax(&boxord[6 * (int64_t)t + 3 + k], ext[(3 + k) * TT_TREES + j]);
        }
    }
    for (int j = threadIdx.x; j < TT_COUNTS; j += TT_BLOCK) {
        const unsigned long long pair = pair_keys[j];
        if (pair != ST_EMPTY_KEY) atomicAdd(&counts[pair], (unsigned long long)pair_sums[j]);
    }
}

// Is this lane the one that takes `key` to global memory for its workgroup?  (true as well when the set has no slot for it.)
__device__ __forceinline__ bool tt_first_in_workgroup(unsigned long long* set, unsigned long long key) {
    unsigned slot = (unsigned)(st_hash64(key) >> 40) & (TT_SET - 1);
    for (int probe = 0; probe < TT_PROBES; probe++, slot = (slot + 1u) & (TT_SET - 1)) {
        unsigned long long prev = set[slot];
        if (prev == ST_EMPTY_KEY) prev = atomicCAS(&set[slot], (unsigned long long)ST_EMPTY_KEY, key);
        if (prev == ST_EMPTY_KEY) return true;
        if (prev == key) return false;
    }
    return true;
}

// true for the one lane that installs `key`.  Linear probing over ALL cap slots (cap a power of two): with at most cap / 2 keys the
// walk ends at the key or at an empty slot.  A walk that met neither would mean the key is not in the set: it is never read as
// "already there" (unreachable while the layout keeps the set half empty).
__device__ __forceinline__ bool tt_install(unsigned long long* table, unsigned long long cap, unsigned long long key) {
    unsigned long long slot = st_hash64(key) & (cap - 1);
    for (unsigned long long probe = 0; probe < cap; probe++) {
        unsigned long long prev = table[slot];
        if (prev == ST_EMPTY_KEY) prev = atomicCAS(&table[slot], (unsigned long long)ST_EMPTY_KEY, key);
        if (prev == ST_EMPTY_KEY) return true;
        if (prev == key) return false;
        slot = (slot + 1ull) & (cap - 1);
    }
    return true;
}

__global__ void __launch_bounds__(TT_BLOCK) k_tt_cells(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ tree,
                                                       const uint8_t* __restrict__ cls, int n_classes, int64_t n_trees, int up, float cell,
                                                       int layers, const unsigned* __restrict__ boxord, unsigned long long* table,
                                                       unsigned long long cap, unsigned long long* area_cells, unsigned long long* profile) {
    __shared__ unsigned long long set[TT_SET];
    for (int j = threadIdx.x; j < TT_SET; j += TT_BLOCK) set[j] = ST_EMPTY_KEY;
    __syncthreads();
    const int h0 = up == 0 ? 1 : 0, h1 = up == 2 ? 1 : 2;
    const int64_t base = (int64_t)blockIdx.x * (TT_TILES * TT_BLOCK);
    for (int tile = 0; tile < TT_TILES; tile++) {
        const int64_t i = base + (int64_t)tile * TT_BLOCK + threadIdx.x;
        if (i >= n) break;
        int t, c;
        float p[3];
        if (!tt_point(pts, tree, cls, n_classes, n_trees, i, &t, &c, p)) continue;
        unsigned long long idx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float d = p[k] - st_ord2f(boxord[6 * (int64_t)t + k]);
            const float f = floorf(d / cell);
            idx[k] = (unsigned long long)(int)fminf(fmaxf(f, 0.0f), TT_MAX_INDEX);  // clamped as a float: an overflowed d has an index too
        }
        const unsigned long long plan = ((unsigned long long)(unsigned)t << 42) | (idx[h1] << 14) | idx[h0];
        if (area_cells && tt_first_in_workgroup(set, plan) && tt_install(table, cap, plan)) atomicAdd(&area_cells[t], 1ull);
        if (profile) {
            const unsigned long long volume = (1ull << 63) | plan | (idx[up] << 28);
            if (tt_first_in_workgroup(set, volume) && tt_install(table, cap, volume)) {
                const int64_t layer = st_min((int64_t)idx[up], (int64_t)layers - 1);
                atomicAdd(&profile[(int64_t)t * layers + layer], 1ull);
            }
        }
    }
}

// --------------------------------------------------------------------------------------- host ---
struct TtLayout {
    unsigned* boxord;
    unsigned long long* table;
    int64_t cap;
};

static void tt_layout(StArena& a, int64_t n, int64_t n_trees, TtLayout* L) {
    L->boxord = a.take<unsigned>(6 * n_trees);
    L->cap = st_next_pow2(4 * n > 16 ? 4 * n : 16);  // two keys per point at worst, at most half full
    L->table = a.take<unsigned long long>(n > 0 ? L->cap : 1);
}

static bool tt_sizes_ok(int64_t n, int64_t n_trees, int layers) {
    return n >= 0 && n < (1ll << 31) && n_trees >= 0 && n_trees < TT_MAX_TREES && layers >= 1 && layers <= 4096;
}

extern "C" int64_t st_tree_tally_workspace_bytes(int64_t n, int64_t n_trees, int layers) {
    if (!tt_sizes_ok(n, n_trees, layers)) return -1;
    StArena a(nullptr, 0);
    TtLayout L;
    tt_layout(a, n, n_trees, &L);
    return a.used;
}

extern "C" int st_tree_tally(const float* pts, int64_t n, const int32_t* tree, const uint8_t* cls, int n_classes, int64_t n_trees, int up,
                             float cell, int layers, float* box, int64_t* counts, int64_t* area_cells, int64_t* profile, void* ws,
                             int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n >= 0 && n < (1ll << 31), "tree_tally: 0 <= points < 2^31 (got %lld)", (long long)n);
    ST_REQUIRE(n_trees >= 0 && n_trees < TT_MAX_TREES, "tree_tally: 0 <= trees < 2^21 (got %lld)", (long long)n_trees);
    ST_REQUIRE(layers >= 1 && layers <= 4096, "tree_tally: 1 <= layers <= 4096 (got %d)", layers);
    ST_REQUIRE(up >= 0 && up <= 2, "tree_tally: the vertical axis is 0, 1 or 2 (got %d)", up);
    ST_REQUIRE(cell > 0.0f && cell <= 3.4028234e38f, "tree_tally: the cell size must be finite and > 0 (got %g)", (double)cell);
    ST_REQUIRE(n_classes >= 1 && n_classes <= 255, "tree_tally: 1 <= classes <= 255 (got %d)", n_classes);
    ST_REQUIRE(n == 0 || (pts && tree), "tree_tally: %lld points need their coordinates and their trees", (long long)n);
    StArena arena(ws, ws_bytes);
    TtLayout L;
    tt_layout(arena, n, n_trees, &L);
    if (!arena.ok() || !ws) {
        st_set_error("tree_tally: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (n_trees == 0) return ST_OK;
    if (!cls) n_classes = 1;
    const unsigned tb = (unsigned)st_div_up(6 * n_trees, TT_BLOCK);
    hipLaunchKernelGGL(k_tt_init, dim3(tb), dim3(TT_BLOCK), 0, stream, L.boxord, n_trees);
    if (counts) (void)hipMemsetAsync(counts, 0, (size_t)(n_trees * n_classes) * sizeof(int64_t), stream);
    if (area_cells) (void)hipMemsetAsync(area_cells, 0, (size_t)n_trees * sizeof(int64_t), stream);
    if (profile) (void)hipMemsetAsync(profile, 0, (size_t)(n_trees * layers) * sizeof(int64_t), stream);
    if (n > 0) {
        const unsigned pb = (unsigned)st_div_up(n, TT_TILES * TT_BLOCK);
        hipLaunchKernelGGL(k_tt_box, dim3(pb), dim3(TT_BLOCK), 0, stream, pts, n, tree, cls, n_classes, n_trees, L.boxord,
                           (unsigned long long*)counts);
        if (area_cells || profile) {
            (void)hipMemsetAsync(L.table, 0xff, (size_t)L.cap * sizeof(unsigned long long), stream);
            hipLaunchKernelGGL(k_tt_cells, dim3(pb), dim3(TT_BLOCK), 0, stream, pts, n, tree, cls, n_classes, n_trees, up, cell, layers,
                               (const unsigned*)L.boxord, L.table, (unsigned long long)L.cap, (unsigned long long*)area_cells,
                               (unsigned long long*)profile);
        }
    }
    if (box) hipLaunchKernelGGL(k_tt_box_out, dim3(tb), dim3(TT_BLOCK), 0, stream, (const unsigned*)L.boxord, n_trees, box);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
