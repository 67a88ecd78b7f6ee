// st_bridge_components: join the kept components of a neighbourhood graph across gaps of at most max_gap.
//
// The reference never finished this (skeleton/connection.py stops half way; data_types/tree.py:connect "only visually gives
// appearance of connection"); a branch cut by occlusion comes back as a trunk plus rootless fragments.  The bridges returned
// here are added to the graph BEFORE the shortest-path stage, which then simply sees fewer, larger components.
//
// Definition (exact; tests/test_bridge.py restates it as a brute force + Kruskal):
//   candidates  all vertex pairs (u, v) in different kept components of one cloud with d2(u, v) <= r2, r2 = max_gap * max_gap
//               formed once in float32 on the host
//   d2          (dx*dx + dy*dy) + dz*dz in float32, dx = p[u].x - p[v].x ..., no contraction (symmetric in u and v)
//   order       strict and total: (bits of d2, lo, hi), lo < hi the ORIGINAL vertex ids
//   bridges     the minimum spanning forest of the component graph under that order (unique); weight = sqrtf(d2)
// Vertices of dropped components are neither queries nor candidates.
//
// Form: Boruvka rounds over a uniform grid (st_grid.h) of the kept vertices, cell = max_gap (a little more: see br_reach).
//   scan     one lane per active vertex, in cell order: the cells its reach touches are read as z-runs of the cell-sorted records,
//            candidates that carry the query's own current label are skipped, the lane keeps its own minimum under the order and
//            offers its d2 to its component (atomicMin on the 32 bits of d2: d2 >= 0, the bits order like the values)
//   pair     the lanes whose d2 IS their component's minimum offer their (lo, hi) (atomicMin on 64 bits).  Two integer minima,
//            two launches: nothing depends on which lane arrives first, and no float atomics
//   hook     one lane per root: the component at the other end of its winning edge becomes its parent -- unless both chose the
//            same edge, then the larger label goes under the smaller.  A strict total order admits no longer cycle.  The
//            component that is hooked records the edge in ITS OWN slot (a component is hooked once in its life): no counter
//            hands out output rows, the output order is the component order
//   flatten  labels of components and vertices follow the parent chains to the roots; the per-component minima are cleared
// A vertex that saw no foreign candidate in round 1 never will (labels only merge): rounds >= 2 run over round 1's boundary
// set, compacted in cell order.  The host reads one 16-byte record per round -- components hooked, boundary size -- and stops
// after the round that hooks nothing: at most ceil(log2 C) + 1 rounds.  Memory: O(m + C) words beside the cell table.
#include "st_common.h"
#include "st_grid.h"

#define BR_BLOCK 256
#define BR_EMPTY32 0xffffffffu
#define BR_EMPTY64 0xffffffffffffffffull
#define BR_MAX_CELLS (1ll << 22)  // cells per cloud at most (16 MiB of cell table); a coarser grid changes the speed, never the result

static inline unsigned br_blocks(int64_t n) {
    const int64_t g = st_div_up(n > 0 ? n : 1, BR_BLOCK);
    return (unsigned)(g < 8192 ? g : 8192);
}
#define BR_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

static inline int64_t br_cells(int64_t m, int nseg) {  // (st_grid_build itself uses at most 128 cells per point)
    return st_min64(BR_MAX_CELLS * (nseg < 1 ? 1 : (nseg > 32 ? 32 : nseg)), 128 * m + 65536);
}

struct BrCounters {
    unsigned hooked;    // components hooked in the current round
    unsigned boundary;  // vertices that saw a foreign candidate in round 1
    unsigned bad;       // malformed input met (a vertex id outside the point array)
    unsigned pad;
};

// component of renumbered vertex k: comp_off[c] <= k < comp_off[c + 1]
__device__ __forceinline__ int br_comp_of(const int32_t* comp_off, int C, int k) {
    int lo = 0, hi = C;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (comp_off[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

// cell of coordinate v along axis a, clamped into the cloud's slab AS A FLOAT (a reach far beyond the box, or a NaN, must not
// reach the integer conversion).  Monotone in v, and equal to st_grid_axis for every finite v: a point p with
// q - reach <= p <= q + reach lies in a cell between cell(q - reach) and cell(q + reach), whatever the roundings inside.
__device__ __forceinline__ int br_axis(const StGrid* g, float v, int a) {
    const int d = a == 0 ? g->seg_dim0 : g->dim[a];
    float c = floorf((v - g->lo[a]) / g->cell);
    c = fminf(fmaxf(c, 0.0f), (float)(d - 1));
    return (int)c;
}

// ----------------------------------------------------------------------------------- set-up ---
// the kept vertices in the renumbered order (components contiguous, clouds contiguous): what the grid is built over
__global__ void __launch_bounds__(BR_BLOCK) k_br_gather(const float* pts, int64_t n, const int32_t* vert_order, int64_t m, float* kpts,
                                                        BrCounters* cnt) {
    BR_LOOP(k, m) {
        const int64_t v = vert_order[k];
        const bool ok = v >= 0 && v < n;
        const float nan = __uint_as_float(0x7fc00000u);  // nobody's neighbour
        kpts[3 * k] = ok ? pts[3 * v] : nan;
        kpts[3 * k + 1] = ok ? pts[3 * v + 1] : nan;
        kpts[3 * k + 2] = ok ? pts[3 * v + 2] : nan;
        if (!ok) atomicAdd(&cnt->bad, 1u);
    }
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_init(int C, int32_t* label, unsigned* best_d2, unsigned long long* best_pair,
                                                      unsigned long long* out_pair, BrCounters* cnt) {
    BR_LOOP(c, C) {
        label[c] = (int32_t)c;
        best_d2[c] = BR_EMPTY32;
        best_pair[c] = BR_EMPTY64;
        out_pair[c] = BR_EMPTY64;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { cnt->hooked = 0u; cnt->boundary = 0u; cnt->bad = 0u; cnt->pad = 0u; }
}

// per record of the cell-sorted list: the component of its vertex (fixed) and that component's current label
__global__ void __launch_bounds__(BR_BLOCK) k_br_vcomp(const float4* recs, int64_t m, const int32_t* comp_off, int C, int32_t* vcomp,
                                                       int32_t* vlabel) {
    BR_LOOP(t, m) {
        const int c = br_comp_of(comp_off, C, (int)__float_as_uint(recs[t].w));
        vcomp[t] = c;
        vlabel[t] = c;
    }
}

// ------------------------------------------------------------------------------------- round ---
// FIRST: every record is a query (active == nullptr, slot a = record t) and the boundary flags are written
template <bool FIRST>
__global__ void __launch_bounds__(BR_BLOCK) k_br_scan(const StGrid* __restrict__ g, const uint32_t* __restrict__ cell_start,
                                                      const float4* __restrict__ recs, const int32_t* __restrict__ vlabel,
                                                      const int32_t* __restrict__ vert_order, const uint32_t* __restrict__ active,
                                                      int64_t n_active, const int32_t* __restrict__ vert_seg_off, int nseg, float r2,
                                                      float reach, unsigned* __restrict__ vbest_d2, unsigned long long* __restrict__ vbest_pair,
                                                      unsigned* __restrict__ best_d2, uint32_t* __restrict__ flags, BrCounters* cnt) {
    BR_LOOP(a, n_active) {
        const uint32_t t = FIRST ? (uint32_t)a : active[a];
        const float4 me = recs[t];
        const int my = vlabel[t];
        const int k = (int)__float_as_uint(me.w);
        unsigned bd = BR_EMPTY32;
        unsigned long long bp = BR_EMPTY64;
        // a vertex with a NaN / infinite coordinate is nobody's neighbour: every distance to it is NaN or infinite, and r2 is finite
        const bool finite = fabsf(me.x) <= 3.0e38f && fabsf(me.y) <= 3.0e38f && fabsf(me.z) <= 3.0e38f;
        if (finite) {
            const unsigned i = (unsigned)vert_order[k];
            const int xoff = st_seg_find(vert_seg_off, nseg, k) * g->seg_dim0;  // the cloud's slab of cells: a search never leaves it
            const int x0 = br_axis(g, me.x - reach, 0), x1 = br_axis(g, me.x + reach, 0);
            const int y0 = br_axis(g, me.y - reach, 1), y1 = br_axis(g, me.y + reach, 1);
            const int z0 = br_axis(g, me.z - reach, 2), z1 = br_axis(g, me.z + reach, 2);
            for (int x = x0; x <= x1; x++)
                for (int y = y0; y <= y1; y++) {
                    const int64_t row = ((int64_t)(xoff + x) * g->dim[1] + y) * g->dim[2];
                    const uint32_t s = cell_start[row + z0], e = cell_start[row + z1 + 1];  // a z-run is contiguous in recs
                    for (uint32_t u = s; u < e; u++) {
                        if (vlabel[u] == my) continue;
                        const float4 q = recs[u];
                        const float dx = me.x - q.x, dy = me.y - q.y, dz = me.z - q.z;
                        float d2 = dx * dx;
                        float tt = dy * dy;
                        d2 = d2 + tt;
                        tt = dz * dz;
                        d2 = d2 + tt;
                        if (!(d2 <= r2)) continue;
                        const unsigned j = (unsigned)vert_order[(int)__float_as_uint(q.w)];
                        const unsigned db = __float_as_uint(d2);  // d2 >= +0: the bits order like the values
                        const unsigned long long pr = i < j ? ((unsigned long long)i << 32) | j : ((unsigned long long)j << 32) | i;
                        if (db < bd || (db == bd && pr < bp)) { bd = db; bp = pr; }
                    }
                }
        }
        vbest_d2[a] = bd;
        vbest_pair[a] = bp;
        if (FIRST) flags[t] = bd != BR_EMPTY32 ? 1u : 0u;
        if (bd != BR_EMPTY32) {
            if (FIRST) atomicAdd(&cnt->boundary, 1u);
            if (best_d2[my] > bd) atomicMin(&best_d2[my], bd);  // (a stale read can only send a lane to the atomic needlessly)
        }
    }
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_pair(const uint32_t* active, int64_t n_active, const int32_t* vlabel,
                                                      const unsigned* vbest_d2, const unsigned long long* vbest_pair,
                                                      const unsigned* best_d2, unsigned long long* best_pair) {
    BR_LOOP(a, n_active) {
        const unsigned bd = vbest_d2[a];
        if (bd == BR_EMPTY32) continue;
        const int my = vlabel[active ? active[a] : (uint32_t)a];
        if (best_d2[my] != bd) continue;
        const unsigned long long pr = vbest_pair[a];
        if (best_pair[my] > pr) atomicMin(&best_pair[my], pr);
    }
}

// next[c]: where component c points after this round -- a hooked root at its new parent, everybody else at its label
__global__ void __launch_bounds__(BR_BLOCK) k_br_hook(int C, const int32_t* label, const unsigned* best_d2, const unsigned long long* best_pair,
                                                      const int32_t* new_id, const int32_t* comp_off, int32_t* next,
                                                      unsigned long long* out_pair, unsigned* out_d2, BrCounters* cnt) {
    BR_LOOP(c, C) {
        int to = label[c];
        if (to == (int)c && best_d2[c] != BR_EMPTY32) {
            const unsigned long long pr = best_pair[c];
            const int ca = label[br_comp_of(comp_off, C, new_id[(unsigned)(pr >> 32)])];
            const int cb = label[br_comp_of(comp_off, C, new_id[(unsigned)(pr & 0xffffffffull)])];
            const int o = ca == (int)c ? cb : ca;  // the root at the other end
            const bool mutual = best_d2[o] != BR_EMPTY32 && best_pair[o] == pr;  // both chose this very edge
            if (o != (int)c && !(mutual && (int)c < o)) {
                to = o;
                out_pair[c] = pr;
                out_d2[c] = best_d2[c];
                atomicAdd(&cnt->hooked, 1u);
            }
        }
        next[c] = to;
    }
}

// lanes [0, C): components; lanes [0, m): records.  Both only READ next (no chain is rewritten while another lane walks it).
__global__ void __launch_bounds__(BR_BLOCK) k_br_flatten(int C, const int32_t* next, int32_t* label, unsigned* best_d2,
                                                         unsigned long long* best_pair, int64_t m, const int32_t* vcomp, int32_t* vlabel) {
    const int64_t total = m > C ? m : (int64_t)C;
    BR_LOOP(t, total) {
        if (t < C) {
            int r = next[t];
            while (next[r] != r) r = next[r];
            label[t] = r;
            best_d2[t] = BR_EMPTY32;
            best_pair[t] = BR_EMPTY64;
        }
        if (t < m) {
            int r = next[vcomp[t]];
            while (next[r] != r) r = next[r];
            vlabel[t] = r;
        }
    }
}

// ------------------------------------------------------------------------- boundary, output ---
__global__ void __launch_bounds__(BR_BLOCK) k_br_compact(const uint32_t* off, int64_t m, uint32_t* active) {
    BR_LOOP(t, m)
        if (off[t + 1] != off[t]) active[off[t]] = (uint32_t)t;
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_outflag(int C, const unsigned long long* out_pair, uint32_t* oflag) {
    BR_LOOP(c, C + 1) oflag[c] = (c < C && out_pair[c] != BR_EMPTY64) ? 1u : 0u;
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_emit(int C, const unsigned long long* out_pair, const unsigned* out_d2, const uint32_t* ooff,
                                                      int64_t cap, int64_t* edges, float* weights) {
    BR_LOOP(c, C) {
        if (out_pair[c] == BR_EMPTY64) continue;
        const int64_t o = ooff[c];
        if (o >= cap) continue;  // (cannot happen: at most C - 1 components are ever hooked, and the host checks cap first)
        edges[2 * o] = (int64_t)(out_pair[c] >> 32);
        edges[2 * o + 1] = (int64_t)(out_pair[c] & 0xffffffffull);
        weights[o] = sqrtf(__uint_as_float(out_d2[c]));
    }
}

// --------------------------------------------------------------------------------------- host ---
struct BrLayout {
    BrCounters* cnt;
    float* kpts;
    StGrid* g;
    uint32_t* cell_start;
    float4* recs;
    int32_t *vcomp, *vlabel;
    unsigned* vbest_d2;
    unsigned long long* vbest_pair;
    uint32_t *flags, *active;
    int32_t *label, *next;
    unsigned *best_d2, *out_d2;
    unsigned long long *best_pair, *out_pair;
    uint32_t* oflag;
    char *gws, *sws;
    int64_t gws_bytes, sws_bytes;
};

static void br_layout(StArena& a, int64_t m, int64_t C, int nseg, BrLayout* L) {
    L->cnt = a.take<BrCounters>(1);
    L->kpts = a.take<float>(3 * m);
    L->g = a.take<StGrid>(1);
    L->cell_start = a.take<uint32_t>(br_cells(m, nseg) + 1);
    L->recs = a.take<float4>(m);
    L->vcomp = a.take<int32_t>(m);
    L->vlabel = a.take<int32_t>(m);
    L->vbest_d2 = a.take<unsigned>(m);
    L->vbest_pair = a.take<unsigned long long>(m);
    L->flags = a.take<uint32_t>(m + 1);
    L->active = a.take<uint32_t>(m);
    L->label = a.take<int32_t>(C);
    L->next = a.take<int32_t>(C);
    L->best_d2 = a.take<unsigned>(C);
    L->out_d2 = a.take<unsigned>(C);
    L->best_pair = a.take<unsigned long long>(C);
    L->out_pair = a.take<unsigned long long>(C);
    L->oflag = a.take<uint32_t>(C + 1);
    L->gws_bytes = st_grid_ws_bytes(m, br_cells(m, nseg));
    L->gws = a.take<char>(L->gws_bytes);
    L->sws_bytes = st_scan_ws_bytes((m > C ? m : C) + 1);
    L->sws = a.take<char>(L->sws_bytes);
}

extern "C" int64_t st_bridge_components_workspace_bytes(int64_t m, int64_t n_comp, int nseg) {
    if (m < 0 || n_comp < 0) return 256;
    StArena a(nullptr, 0);
    BrLayout L;
    br_layout(a, m, n_comp, nseg, &L);
    return a.used;
}

extern "C" int st_bridge_components_seg(const float* pts, int64_t n, const int32_t* vert_order, int64_t m, const int32_t* new_id,
                                        const int32_t* comp_off, int64_t n_comp, const int32_t* vert_seg_off, int nseg, float max_gap,
                                        int64_t* edges, float* weights, int64_t cap, int64_t* n_bridges_host, int64_t* stats_host,
                                        void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n_bridges_host != nullptr, "bridge_components: the bridge count is read back (n_bridges_host is NULL)");
    *n_bridges_host = 0;
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0;
    ST_REQUIRE(n >= 0 && m >= 0 && m <= n && n < (1ll << 31) && n_comp >= 0 && n_comp <= m, "bridge_components: 0 <= components <= kept vertices <= vertices < 2^31");
    ST_REQUIRE(nseg >= 1 && nseg <= ST_MAX_SEG && (nseg == 1 || vert_seg_off), "bridge_components: 1 <= clouds per batch <= %d", ST_MAX_SEG);
    // nothing to join: no launch at all
    if (m == 0 || n_comp <= 1 || !(max_gap > 0.0f)) return ST_OK;
    const float r2 = max_gap * max_gap;  // the bound of the definition, formed once
    ST_REQUIRE(r2 <= 3.0e38f, "bridge_components: max_gap^2 must be a finite float32 (got max_gap = %g)", (double)max_gap);
    ST_REQUIRE(cap >= n_comp - 1, "bridge_components: room for components - 1 bridges needed");
    if (nseg == 1) vert_seg_off = nullptr;
    // |dx| <= max_gap up to the roundings of dx*dx <= r2 (a few parts in 10^7): the reach is a little longer, and so is the cell
    const float reach = max_gap * 1.0001f;
    const int C = (int)n_comp;
    StArena a(ws, ws_bytes);
    BrLayout L;
    br_layout(a, m, n_comp, nseg, &L);
    if (!a.ok() || !ws) { st_set_error("bridge_components: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)a.used); return ST_ERR_WORKSPACE; }

    hipLaunchKernelGGL(k_br_init, dim3(br_blocks(C)), dim3(BR_BLOCK), 0, stream, C, L.label, L.best_d2, L.best_pair, L.out_pair, L.cnt);
    hipLaunchKernelGGL(k_br_gather, dim3(br_blocks(m)), dim3(BR_BLOCK), 0, stream, pts, n, vert_order, m, L.kpts, L.cnt);
    ST_TRY(st_grid_build(L.kpts, m, reach, br_cells(m, nseg), L.g, L.cell_start, L.recs, L.gws, L.gws_bytes, stream, 0.0f, nullptr, 0,
                         vert_seg_off, nseg));
    hipLaunchKernelGGL(k_br_vcomp, dim3(br_blocks(m)), dim3(BR_BLOCK), 0, stream, (const float4*)L.recs, m, comp_off, C, L.vcomp, L.vlabel);

    int64_t n_active = m, rounds = 0, boundary = 0, total = 0;
    const uint32_t* active = nullptr;
    for (;;) {
        if (rounds == 0)
            hipLaunchKernelGGL((k_br_scan<true>), dim3(br_blocks(n_active)), dim3(BR_BLOCK), 0, stream, (const StGrid*)L.g,
                               (const uint32_t*)L.cell_start, (const float4*)L.recs, (const int32_t*)L.vlabel, vert_order, active, n_active,
                               vert_seg_off, nseg, r2, reach, L.vbest_d2, L.vbest_pair, L.best_d2, L.flags, L.cnt);
        else
            hipLaunchKernelGGL((k_br_scan<false>), dim3(br_blocks(n_active)), dim3(BR_BLOCK), 0, stream, (const StGrid*)L.g,
                               (const uint32_t*)L.cell_start, (const float4*)L.recs, (const int32_t*)L.vlabel, vert_order, active, n_active,
                               vert_seg_off, nseg, r2, reach, L.vbest_d2, L.vbest_pair, L.best_d2, L.flags, L.cnt);
        hipLaunchKernelGGL(k_br_pair, dim3(br_blocks(n_active)), dim3(BR_BLOCK), 0, stream, active, n_active, (const int32_t*)L.vlabel,
                           (const unsigned*)L.vbest_d2, (const unsigned long long*)L.vbest_pair, (const unsigned*)L.best_d2, L.best_pair);
        hipLaunchKernelGGL(k_br_hook, dim3(br_blocks(C)), dim3(BR_BLOCK), 0, stream, C, (const int32_t*)L.label, (const unsigned*)L.best_d2,
                           (const unsigned long long*)L.best_pair, new_id, comp_off, L.next, L.out_pair, L.out_d2, L.cnt);
        BrCounters h;
        (void)hipMemcpyAsync(&h, L.cnt, sizeof(BrCounters), hipMemcpyDeviceToHost, stream);
        st_stream_wait(stream);  // the round's read-back
        ST_CHECK_LAUNCH();
        rounds++;
        ST_REQUIRE(h.bad == 0u, "bridge_components: vert_order names a vertex outside the point array");
        if (rounds == 1) boundary = h.boundary;
        if (h.hooked == 0u) break;
        total += h.hooked;
        ST_REQUIRE(total <= n_comp - 1 && rounds <= 64, "bridge_components: more hooks than components (internal error)");
        hipLaunchKernelGGL(k_br_flatten, dim3(br_blocks(m > C ? m : C)), dim3(BR_BLOCK), 0, stream, C, (const int32_t*)L.next, L.label,
                           L.best_d2, L.best_pair, m, (const int32_t*)L.vcomp, L.vlabel);
        (void)hipMemsetAsync(&L.cnt->hooked, 0, sizeof(unsigned), stream);
        if (rounds == 1) {  // later rounds: the boundary set only, in cell order
            (void)hipMemsetAsync(L.flags + m, 0, sizeof(uint32_t), stream);
            ST_TRY(st_exclusive_scan_u32(L.flags, L.flags, m + 1, nullptr, L.sws, L.sws_bytes, stream));
            hipLaunchKernelGGL(k_br_compact, dim3(br_blocks(m)), dim3(BR_BLOCK), 0, stream, (const uint32_t*)L.flags, m, L.active);
            active = L.active;
            n_active = boundary;
        }
    }
    if (stats_host) { stats_host[0] = rounds; stats_host[1] = boundary; stats_host[2] = total; }
    if (total == 0) return ST_OK;
    hipLaunchKernelGGL(k_br_outflag, dim3(br_blocks(C + 1)), dim3(BR_BLOCK), 0, stream, C, (const unsigned long long*)L.out_pair, L.oflag);
    ST_TRY(st_exclusive_scan_u32(L.oflag, L.oflag, (int64_t)C + 1, nullptr, L.sws, L.sws_bytes, stream));
    hipLaunchKernelGGL(k_br_emit, dim3(br_blocks(C)), dim3(BR_BLOCK), 0, stream, C, (const unsigned long long*)L.out_pair,
                       (const unsigned*)L.out_d2, (const uint32_t*)L.oflag, cap, edges, weights);
    ST_CHECK_LAUNCH();
    *n_bridges_host = total;
    return ST_OK;
}
