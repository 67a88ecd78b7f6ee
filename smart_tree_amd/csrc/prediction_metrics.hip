// st_prediction_metrics: how good the network's per-point predictions of one batch are, per tree, in ONE pass over the rows
// st_loss_forward reads: the confusion matrix of the class head, the radius and direction errors, the distance between the
// predicted and the labelled medial point (the quantity the skeleton stage consumes), how many points land within a multiple
// of their branch radius, and the relative errors by radius bin.
//
// Replaces  nothing in the reference (its only feedback on the predictions was wandb images); as torch expressions the same
//           figures are a score of launches with boolean compactions per batch and per tree, and float sums whose order is
//           not fixed.  Here a row is read once ((10 + C) * 4 + 1 bytes, nothing written per row): HBM-bound.
//
// Per row i, float32 in exactly this order, contraction off (tests/metrics_oracle.py restates it).  Steps shared with
// k_loss_partial (loss.hip) use its expressions, so a metric and its loss term cover the same rows.
//   selected      mask == NULL or mask[i] != 0; an unselected row touches nothing                              rows += 1
//   target class  tcf = t[4]; valid iff tcf > -1 && tcf < C; tc = (int)tcf (truncation).  Invalid: bad_class += 1, nothing else
//   prediction    pc = the first NaN logit if any, otherwise the first largest logit (torch.argmax)   confusion[tc][pc] += 1
//   vector row    vector_class < 0 or tc == vector_class; the rest is for vector rows only
//   radius        r_gt = t[0]; r_pred = target_radius_log ? expf(radius[i]) : radius[i]; dr = fabsf(r_pred - r_gt)
//   direction     np = fmaxf(sqrtf(px*px + py*py + pz*pz), 1e-8f), nq likewise; p^ = p / np, q^ = q / nq (per component)
//                 cs = p^x*q^x + p^y*q^y + p^z*q^z, clamped to [-1, 1]; ang = acosf(cs)
//   medial error  e = r_pred * p^ - r_gt * q^ (per component); err = sqrtf((ex*ex + ey*ey) + ez*ez)
//   guard         any of dr, dr / r_gt, ang, err, err / r_gt not finite: bad_vector += 1, nothing else
//   otherwise     vector_rows += 1; sums += {dr, dr / r_gt, ang, err, err / r_gt}; within[j] += err <= thr[j] * r_gt;
//                 bin = #{edges e: r_gt >= e}; bin_count[bin] += 1; bin_dr_rel[bin] += dr / r_gt; bin_err_rel[bin] += err / r_gt
//
// Record of a segment (include/smarttree_hip.h):  int64  confusion[C*C] | bad_class | vector_rows | bad_vector | rows |
//   within[T] | bin_count[NB];   double  sum dr | sum dr/r_gt | sum ang | sum err | sum err/r_gt | bin_dr_rel[NB] | bin_err_rel[NB].
//
// Reduction.  A workgroup owns one tile of PM_TILE consecutive rows of ONE segment, counted from the segment's first row (the
// last tile of a segment is short): tile -> (segment, first row) comes from the offsets in the argument block.  Integers: LDS
// counters private to the workgroup (ds_add_u32), one global 64-bit integer atomic per non-zero counter at the end.  Doubles:
// every float32 term widened, lane -> wavefront (shuffles) -> workgroup (LDS) -> the tile's slot in the workspace; k_pm_final adds
// a segment's slots with lane l taking tiles l, l + 64, ... in order and the same shuffle tree.  No float atomics.  A record is a
// function of the segment's rows alone: the same bits when the segment is evaluated on its own, and from call to call.
// A lane cannot index its bin accumulators at run time without spilling them, so every row adds (bin == b ? term : 0.0) to all
// of them: the kernel is instantiated for 8 and for 16 bins.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md "Evaluation: per-point predictions".
#include "st_grid.h"  // ST_MAX_SEG

#define PM_BLOCK 256
#define PM_TILE 2048  // rows per workgroup: eight per lane between two epilogues
#define PM_MAX_CLASSES 16
#define PM_MAX_THR 16
#define PM_MAX_BINS 16
#define PM_SUMS 5
#define PM_SCALARS 4  // bad_class, vector_rows, bad_vector, rows
#define PM_LDS_SCALARS (PM_MAX_CLASSES * PM_MAX_CLASSES)
#define PM_LDS_WITHIN (PM_LDS_SCALARS + PM_SCALARS)
#define PM_LDS_BINS (PM_LDS_WITHIN + PM_MAX_THR)
#define PM_LDS_INTS (PM_LDS_BINS + PM_MAX_BINS)

struct PmArgs {  // host values travel by value: the call checks them and needs no upload
    const float* radius;     // [n]     predicted (log) radius
    const float* direction;  // [n, 3]
    const float* class_l;    // [n, C]
    const float* targets;    // [n, 5]  radius, direction xyz, class id
    const uint8_t* mask;     // [n] or null
    int64_t seg_off[ST_MAX_SEG + 1];
    int32_t tile_off[ST_MAX_SEG + 1];  // first tile of every segment; [n_seg] = all tiles
    float thr[PM_MAX_THR];
    float edges[PM_MAX_BINS - 1];
    int n_seg, n_classes, n_thr, n_bins, vector_class, target_radius_log;
};

__device__ __forceinline__ double pm_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ bool pm_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

template <int NB>
__global__ void __launch_bounds__(PM_BLOCK) k_pm_tally(PmArgs A, unsigned long long* __restrict__ ints, double* __restrict__ partial) {
    __shared__ unsigned s_cnt[PM_LDS_INTS];
    __shared__ double s_sum[PM_BLOCK / 64][PM_SUMS + 2 * NB];
    const int tid = threadIdx.x;
    for (int j = tid; j < PM_LDS_INTS; j += PM_BLOCK) s_cnt[j] = 0u;
    // the segment of this tile: the last one whose first tile is <= blockIdx.x (an empty segment shares its successor's)
    int seg = 0;
    for (int s = 1; s < A.n_seg; s++)
        if (A.tile_off[s] <= (int)blockIdx.x) seg = s;
    const int64_t row0 = A.seg_off[seg] + (int64_t)((int)blockIdx.x - A.tile_off[seg]) * PM_TILE;
    const int64_t seg_end = A.seg_off[seg + 1];
    const int64_t row1 = row0 + PM_TILE < seg_end ? row0 + PM_TILE : seg_end;
    const int C = A.n_classes, nb = A.n_bins;
    __syncthreads();

    double acc[PM_SUMS], acc_dr[NB], acc_err[NB];
#pragma unroll
    for (int k = 0; k < PM_SUMS; k++) acc[k] = 0.0;
#pragma unroll
    for (int b = 0; b < NB; b++) acc_dr[b] = acc_err[b] = 0.0;
    unsigned n_rows = 0u, n_vec = 0u, n_bad_class = 0u, n_bad_vec = 0u;
    for (int64_t i = row0 + tid; i < row1; i += PM_BLOCK) {
        if (A.mask && !A.mask[i]) continue;
        n_rows++;
        const float* t = A.targets + 5 * i;
        const float tcf = t[4];
        if (!(tcf > -1.0f && tcf < (float)C)) {  // as loss.hip: a NaN / infinite id is an id outside the logits
            n_bad_class++;
            continue;
        }
        const int tc = (int)tcf;
        const float* z = A.class_l + (int64_t)C * i;
        float best = z[0];
        int pc = 0;
        for (int k = 1; k < C; k++) {
            const float v = z[k];
            if (best == best && (v > best || v != v)) { best = v; pc = k; }  // a NaN wins once and is never replaced
        }
        atomicAdd(&s_cnt[tc * C + pc], 1u);
        if (A.vector_class >= 0 && tc != A.vector_class) continue;
        const float r_gt = t[0];
        const float r_in = A.radius[i];
        const float r_pred = A.target_radius_log ? expf(r_in) : r_in;
        const float dr = fabsf(r_pred - r_gt);
        const float* d = A.direction + 3 * i;
        const float px = d[0], py = d[1], pz = d[2], qx = t[1], qy = t[2], qz = t[3];
        const float np = fmaxf(sqrtf(px * px + py * py + pz * pz), 1e-8f), nq = fmaxf(sqrtf(qx * qx + qy * qy + qz * qz), 1e-8f);
        const float ux = px / np, uy = py / np, uz = pz / np, hx = qx / nq, hy = qy / nq, hz = qz / nq;
        float cs = ux * hx + uy * hy + uz * hz;
        cs = cs < -1.0f ? -1.0f : (cs > 1.0f ? 1.0f : cs);
        const float ang = acosf(cs);
        const float ex = r_pred * ux - r_gt * hx, ey = r_pred * uy - r_gt * hy, ez = r_pred * uz - r_gt * hz;
        const float err = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float dr_rel = dr / r_gt, err_rel = err / r_gt;
        if (!(pm_finite(dr) && pm_finite(dr_rel) && pm_finite(ang) && pm_finite(err) && pm_finite(err_rel))) {
            n_bad_vec++;
            continue;
        }
        n_vec++;
        acc[0] += (double)dr;
        acc[1] += (double)dr_rel;
        acc[2] += (double)ang;
        acc[3] += (double)err;
        acc[4] += (double)err_rel;
        for (int j = 0; j < A.n_thr; j++)
            if (err <= A.thr[j] * r_gt) atomicAdd(&s_cnt[PM_LDS_WITHIN + j], 1u);
        int bin = 0;
        for (int e = 0; e < nb - 1; e++) bin += r_gt >= A.edges[e] ? 1 : 0;
        atomicAdd(&s_cnt[PM_LDS_BINS + bin], 1u);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            acc_dr[b] += bin == b ? (double)dr_rel : 0.0;
            acc_err[b] += bin == b ? (double)err_rel : 0.0;
        }
    }
    if (n_bad_class) atomicAdd(&s_cnt[PM_LDS_SCALARS + 0], n_bad_class);
    if (n_vec) atomicAdd(&s_cnt[PM_LDS_SCALARS + 1], n_vec);
    if (n_bad_vec) atomicAdd(&s_cnt[PM_LDS_SCALARS + 2], n_bad_vec);
    if (n_rows) atomicAdd(&s_cnt[PM_LDS_SCALARS + 3], n_rows);

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < PM_SUMS; k++) {
        const double w = pm_wave_sum(acc[k]);
        if (lane == 0) s_sum[wave][k] = w;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        if (b < nb) {  // workgroup-uniform
            const double wd = pm_wave_sum(acc_dr[b]), we = pm_wave_sum(acc_err[b]);
            if (lane == 0) { s_sum[wave][PM_SUMS + b] = wd; s_sum[wave][PM_SUMS + NB + b] = we; }
        }
    }
    __syncthreads();
    const int ns = PM_SUMS + 2 * nb;
    if (tid < ns) {
        const int k = tid < PM_SUMS + nb ? tid : tid - nb + NB;  // the record packs the two bin arrays, the LDS rows do not
        double v = 0.0;
        for (int w = 0; w < PM_BLOCK / 64; w++) v += s_sum[w][k];
        partial[(int64_t)blockIdx.x * ns + tid] = v;
    }
    const int cc = C * C;
    unsigned long long* rec = ints + (int64_t)seg * (cc + PM_SCALARS + A.n_thr + nb);
    for (int j = tid; j < PM_LDS_INTS; j += PM_BLOCK) {
        const unsigned c = s_cnt[j];
        if (!c) continue;
        const int at = j < PM_LDS_SCALARS ? j : (j < PM_LDS_WITHIN ? cc + (j - PM_LDS_SCALARS)
                     : (j < PM_LDS_BINS ? cc + PM_SCALARS + (j - PM_LDS_WITHIN) : cc + PM_SCALARS + A.n_thr + (j - PM_LDS_BINS)));
        atomicAdd(&rec[at], (unsigned long long)c);
    }
}

// One workgroup per segment: wavefront w adds sums w, w + 4, ...; lane l the tiles l, l + 64, ... of the segment in order, then
// the shuffle tree.  The order is a function of the segment's tile count.  A segment without tiles gets zeros.
__global__ void __launch_bounds__(PM_BLOCK) k_pm_final(PmArgs A, const double* __restrict__ partial, double* __restrict__ sums) {
    const int seg = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ns = PM_SUMS + 2 * A.n_bins;
    const int64_t t0 = A.tile_off[seg], nt = A.tile_off[seg + 1] - A.tile_off[seg];
    for (int k = wave; k < ns; k += PM_BLOCK / 64) {
        double v = 0.0;
        for (int64_t t = lane; t < nt; t += 64) v += partial[(t0 + t) * ns + k];
        v = pm_wave_sum(v);
        if (lane == 0) sums[(int64_t)seg * ns + k] = v;
    }
}

static bool pm_limits(int n_classes, int n_thr, int n_bins) {
    return n_classes >= 1 && n_classes <= PM_MAX_CLASSES && n_thr >= 0 && n_thr <= PM_MAX_THR && n_bins >= 1 && n_bins <= PM_MAX_BINS;
}
static int64_t pm_tiles_bound(int64_t n, int n_seg) { return st_div_up(n > 0 ? n : 0, PM_TILE) + (n_seg > 0 ? n_seg : 0); }

// -1 when a limit is exceeded
extern "C" int64_t st_prediction_metrics_tally_ints(int n_classes, int n_thr, int n_bins) {
    if (!pm_limits(n_classes, n_thr, n_bins)) return -1;
    return (int64_t)n_classes * n_classes + PM_SCALARS + n_thr + n_bins;
}
extern "C" int64_t st_prediction_metrics_tally_sums(int n_bins) {
    if (n_bins < 1 || n_bins > PM_MAX_BINS) return -1;
    return PM_SUMS + 2 * n_bins;
}
// enough for any split of n rows into n_seg segments: every segment ends in at most one short tile
extern "C" int64_t st_prediction_metrics_workspace_bytes(int64_t n, int n_seg, int n_bins) {
    if (n < 0 || n_seg < 1 || n_seg > ST_MAX_SEG || n_bins < 1 || n_bins > PM_MAX_BINS) return -1;
    StArena a(nullptr, 0);
    a.take<double>(pm_tiles_bound(n, n_seg) * (PM_SUMS + 2 * n_bins));
    return a.used;
}

extern "C" int st_prediction_metrics(const float* radius, const float* direction, const float* class_l, int n_classes,
                                     const float* targets, int target_cols, const uint8_t* mask, int64_t n,
                                     const int64_t* seg_off_host, int n_seg, int vector_class, int target_radius_log,
                                     const float* thr_host, int n_thr, const float* edges_host, int n_edges, int64_t* tally_ints,
                                     double* tally_sums, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int n_bins = n_edges + 1;
    ST_REQUIRE(n >= 0 && n < (1ll << 40), "prediction metrics: bad row count %lld", (long long)n);
    ST_REQUIRE(target_cols == 5, "prediction metrics: targets must be [n, 5] = radius, direction xyz, class (got %d columns)", target_cols);
    ST_REQUIRE(n_classes >= 1 && n_classes <= PM_MAX_CLASSES, "prediction metrics: 1 <= classes <= %d (got %d)", PM_MAX_CLASSES, n_classes);
    ST_REQUIRE(n_thr >= 0 && n_thr <= PM_MAX_THR, "prediction metrics: 0 .. %d thresholds (got %d)", PM_MAX_THR, n_thr);
    ST_REQUIRE(n_edges >= 0 && n_bins <= PM_MAX_BINS, "prediction metrics: 0 .. %d radius edges (got %d)", PM_MAX_BINS - 1, n_edges);
    ST_REQUIRE(n_seg >= 1 && n_seg <= ST_MAX_SEG, "prediction metrics: 1 .. %d segments per call (got %d)", ST_MAX_SEG, n_seg);
    ST_REQUIRE(seg_off_host || n_seg == 1, "prediction metrics: %d segments need their offsets", n_seg);
    ST_REQUIRE((thr_host || n_thr == 0) && (edges_host || n_edges == 0), "prediction metrics: null thresholds or edges");
    ST_REQUIRE(tally_ints && tally_sums, "prediction metrics: null tally");
    ST_REQUIRE(n == 0 || (radius && direction && class_l && targets), "prediction metrics: null input");
    PmArgs A;
    memset(&A, 0, sizeof(A));
    A.radius = radius; A.direction = direction; A.class_l = class_l; A.targets = targets; A.mask = mask;
    A.n_seg = n_seg; A.n_classes = n_classes; A.n_thr = n_thr; A.n_bins = n_bins;
    A.vector_class = vector_class; A.target_radius_log = target_radius_log;
    for (int j = 0; j < n_thr; j++) {
        ST_REQUIRE(thr_host[j] == thr_host[j], "prediction metrics: threshold %d is NaN", j);
        A.thr[j] = thr_host[j];
    }
    for (int e = 0; e < n_edges; e++) {
        ST_REQUIRE(fabsf(edges_host[e]) <= 3.402823466e+38f, "prediction metrics: radius edge %d is not finite", e);
        ST_REQUIRE(e == 0 || edges_host[e] > edges_host[e - 1], "prediction metrics: radius edges must strictly ascend (edge %d: %g after %g)",
                   e, (double)edges_host[e], (double)edges_host[e - 1]);
        A.edges[e] = edges_host[e];
    }
    if (seg_off_host) {
        ST_REQUIRE(seg_off_host[0] == 0, "prediction metrics: segment offsets must start at 0 (got %lld)", (long long)seg_off_host[0]);
        ST_REQUIRE(seg_off_host[n_seg] == n, "prediction metrics: segment offsets must end at n = %lld (got %lld)", (long long)n,
                   (long long)seg_off_host[n_seg]);
    }
    for (int s = 0; s < n_seg; s++) {
        const int64_t lo = seg_off_host ? seg_off_host[s] : 0, hi = seg_off_host ? seg_off_host[s + 1] : n;
        ST_REQUIRE(hi >= lo, "prediction metrics: decreasing segment offset at segment %d (%lld -> %lld)", s, (long long)lo, (long long)hi);
        A.seg_off[s] = lo;
        A.seg_off[s + 1] = hi;
        A.tile_off[s + 1] = A.tile_off[s] + (int32_t)st_div_up(hi - lo, PM_TILE);
    }
    const int64_t tiles = A.tile_off[n_seg];
    const int ns = PM_SUMS + 2 * n_bins;
    double* partial = nullptr;
    if (tiles > 0) {
        StArena arena(ws, ws_bytes);
        partial = arena.take<double>(tiles * ns);
        if (!arena.ok() || !partial) {
            st_set_error("prediction metrics: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
            return ST_ERR_WORKSPACE;
        }
    }
    (void)hipMemsetAsync(tally_ints, 0, (size_t)n_seg * (size_t)(n_classes * n_classes + PM_SCALARS + n_thr + n_bins) * sizeof(int64_t), stream);
    if (tiles > 0) {
        if (n_bins <= 8)
            hipLaunchKernelGGL(k_pm_tally<8>, dim3((unsigned)tiles), dim3(PM_BLOCK), 0, stream, A, (unsigned long long*)tally_ints, partial);
        else
            hipLaunchKernelGGL(k_pm_tally<16>, dim3((unsigned)tiles), dim3(PM_BLOCK), 0, stream, A, (unsigned long long*)tally_ints, partial);
    }
    hipLaunchKernelGGL(k_pm_final, dim3((unsigned)n_seg), dim3(PM_BLOCK), 0, stream, A, (const double*)partial, tally_sums);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
