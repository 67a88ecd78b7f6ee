// Labelled synthetic tree clouds sampled on the device (st_synth_points_seg): B <= 64 trees in one launch, every point
// with its class, its medial vector, its branch id and the table row it was drawn from.
//
// Replaces  the external `synthetic-trees` download of the reference's README (its training set) as the source of labelled
//           trees, and the host sampler smart_tree_amd/synthetic.py:sample_tree_cloud + the upload of its result.
// The geometry model and the meaning of every label are sample_tree_cloud's; the random stream and the foliage draw are not
// (DESIGN.md "Dataset: synthetic trees on the device").
//
// Table row of a segment (16 x 4 bytes, smart_tree_amd/dataset/synthetic.py:segment_table):
//   [0..3] ax ay az ra   [4..7] bx by bz rb   [8..11] ux uy uz branch-id (int32 bits)   [12..15] vx vy vz 0
// cdf[j] (uint32) = floor(2^32 * area[0..j] / area[all]), the tree's last entry 0xFFFFFFFF.
//
// Randomness: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds),
// key = (seed low, seed high) of the tree, counter = (i, k, 0, 0) for draw block k of the tree's point i (local index).
//   block  word  use
//     0     0    class: foliage iff the tree has tips and (w < fol_thr or fol_thr == 0xFFFFFFFF)
//     0     1    branch: segment = first j with cdf[j] > w (the last segment when there is none);  foliage: tip = w % n_tips
//     0     2    branch: t = U(w)                                                                   foliage: unused
//     0     3    branch: theta = 2 pi * U(w)                                                        foliage: unused
//     1     0,1  normal pair (n0, n1) = Box-Muller(w0, w1):  n0 -> x, n1 -> y
//     1     2,3  normal pair (n2, - ) = Box-Muller(w2, w3):  n2 -> z, the sine half is unused
//   U(w) = (w >> 8) * 2^-24;   Box-Muller(wa, wb): m = sqrtf(-2 * logf(((wa >> 8) + 1) * 2^-24)),
//   phi = 2 pi * (((wb >> 8) + 1) * 2^-24), pair = (m * cosf(phi), m * sinf(phi)).
//
// Float32 arithmetic, in this order, contraction off, an FMA only where fmaf is written:
//   branch:  c = cosf(theta), s = sinf(theta);  q = fmaf(s, v, c * u) per axis (the radial unit vector)
//            r = fmaf(rb, t, ra * (1 - t));  p = fmaf(t, b - a, a);  surface = fmaf(r, q, p)
//            xyz = fmaf(noise, n, surface);  medial_vector = -(r * q)   (the un-noised surface point to its axis point)
//   foliage: xyz = fmaf(foliage_sigma, n, tip);  medial_vector = 0;  branch_ids = -1;  segment = -1
//
// Traffic: 36 bytes written per point (less for null outputs), 64 + 4 * log2(S) bytes read per branch point from a table that
// stays in L2 (a depth-7 tree: <= 3.3k rows, 210 KB).  The cdf of the tree that owns the workgroup's first point is staged in
// LDS (<= SY_LDS_CDF entries, 16 KB; a larger table is searched in global memory) -- the rows would not fit; points of any
// other tree the workgroup straddles search that tree's cdf in global memory.  Bound by the HBM writes and ~7 transcendentals.
#include "st_common.h"
#include "st_philox.h"

#define SY_BLOCK 256
#define SY_PPT 8            // points per thread: one cdf staging per 2048 points
#define SY_MAX_TREES 64
#define SY_LDS_CDF 4096

struct SyTrees {  // host values, passed by value: the launch needs no upload and no workspace
    int32_t tab_off[SY_MAX_TREES + 1], tip_off[SY_MAX_TREES + 1], pt_off[SY_MAX_TREES + 1];
    uint32_t seed_lo[SY_MAX_TREES], seed_hi[SY_MAX_TREES], fol_thr[SY_MAX_TREES];
    float noise[SY_MAX_TREES], sigma[SY_MAX_TREES];
    int32_t n_trees;
};

// First j in [0, n) with cdf[j] > w; n - 1 when there is none (w == 0xFFFFFFFF).  n >= 1.
__device__ __forceinline__ int sy_pick(const uint32_t* cdf, int n, uint32_t w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > w) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(SY_BLOCK) k_synth_points(SyTrees T, int64_t n_points, const float4* __restrict__ table,
                                                           const uint32_t* __restrict__ cdf, const float* __restrict__ tips,
                                                           float* __restrict__ xyz, float* __restrict__ mv, float* __restrict__ class_l,
                                                           int32_t* __restrict__ branch_ids, int32_t* __restrict__ segment) {
    __shared__ uint32_t s_cdf[SY_LDS_CDF];
    __shared__ int32_t s_pt[SY_MAX_TREES + 1];
    const int tid = threadIdx.x;
    const int B = T.n_trees;
    const int64_t base = (int64_t)blockIdx.x * (SY_BLOCK * SY_PPT);
    if (tid <= B) s_pt[tid] = T.pt_off[tid];
    // the owner of the workgroup's first point: the last tree whose offset is <= base (an empty tree shares its successor's
    // offset, so the last one is the owner).  Workgroup-uniform.
    int s0 = 0;
    for (int s = 1; s < B; s++)
        if ((int64_t)T.pt_off[s] <= base) s0 = s;
    const int n0 = T.tab_off[s0 + 1] - T.tab_off[s0];
    const bool staged = n0 <= SY_LDS_CDF;
    if (staged)
        for (int j = tid; j < n0; j += SY_BLOCK) s_cdf[j] = cdf[(int64_t)T.tab_off[s0] + j];
    __syncthreads();

    for (int k = 0; k < SY_PPT; k++) {
        const int64_t g = base + (int64_t)k * SY_BLOCK + tid;  // consecutive lanes, consecutive points
        if (g >= n_points) return;
        int s = s0;  // the last tree with pt_off[s] <= g; it is never before s0
        {
            int lo = s0, hi = B;  // pt_off[lo] <= g < pt_off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)s_pt[mid] <= g) lo = mid; else hi = mid;
            }
            s = lo;
        }
        const uint32_t i = (uint32_t)(g - (int64_t)s_pt[s]);
        // per-tree values by a wave-varying index: read from the argument block (constant memory), s is the same for
        // all but a few lanes of a workgroup
        const uint32_t k0 = T.seed_lo[s], k1 = T.seed_hi[s], thr = T.fol_thr[s];
        const int tab0 = T.tab_off[s], n_seg = T.tab_off[s + 1] - tab0;
        const int tip0 = T.tip_off[s], n_tips = T.tip_off[s + 1] - tip0;
        const SyWords d = sy_philox(i, 0u, 0u, 0u, k0, k1);
        const SyWords e = sy_philox(i, 1u, 0u, 0u, k0, k1);
        float nx, ny, nz, unused;
        sy_normal_pair(e.w0, e.w1, nx, ny);
        sy_normal_pair(e.w2, e.w3, nz, unused);
        const bool foliage = n_tips > 0 && (d.w0 < thr || thr == 0xFFFFFFFFu);
        float x, y, z, mx = 0.0f, my = 0.0f, mz = 0.0f;
        int32_t bid = -1, row = -1;
        if (foliage) {
            const int64_t tip = (int64_t)tip0 + (int64_t)(d.w1 % (uint32_t)n_tips);
            const float sg = T.sigma[s];
            x = fmaf(sg, nx, tips[3 * tip]);
            y = fmaf(sg, ny, tips[3 * tip + 1]);
            z = fmaf(sg, nz, tips[3 * tip + 2]);
        } else {
            const int j = (staged && s == s0) ? sy_pick(s_cdf, n_seg, d.w1) : sy_pick(cdf + tab0, n_seg, d.w1);
            row = tab0 + j;
            const float4 A = table[4 * (int64_t)row], Bq = table[4 * (int64_t)row + 1];
            const float4 U = table[4 * (int64_t)row + 2], V = table[4 * (int64_t)row + 3];
            bid = (int32_t)__float_as_uint(U.w);
            const float t = sy_uniform(d.w2);
            const float theta = SY_TWO_PI * sy_uniform(d.w3);
            const float c = cosf(theta), sn = sinf(theta);
            const float qx = fmaf(sn, V.x, c * U.x), qy = fmaf(sn, V.y, c * U.y), qz = fmaf(sn, V.z, c * U.z);
            const float r = fmaf(Bq.w, t, A.w * (1.0f - t));
            const float px = fmaf(t, Bq.x - A.x, A.x), py = fmaf(t, Bq.y - A.y, A.y), pz = fmaf(t, Bq.z - A.z, A.z);
            const float ns = T.noise[s];
            x = fmaf(ns, nx, fmaf(r, qx, px));
            y = fmaf(ns, ny, fmaf(r, qy, py));
            z = fmaf(ns, nz, fmaf(r, qz, pz));
            mx = -(r * qx);
            my = -(r * qy);
            mz = -(r * qz);
        }
        if (xyz) { xyz[3 * g] = x; xyz[3 * g + 1] = y; xyz[3 * g + 2] = z; }
        if (mv) { mv[3 * g] = mx; mv[3 * g + 1] = my; mv[3 * g + 2] = mz; }
        if (class_l) class_l[g] = foliage ? 1.0f : 0.0f;
        if (branch_ids) branch_ids[g] = bid;
        if (segment) segment[g] = row;
    }
}

// Test-only export: one Philox4x32-10 block on the host, the same function the kernel calls.
extern "C" void st_synth_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    const SyWords w = sy_philox(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    out[0] = w.w0; out[1] = w.w1; out[2] = w.w2; out[3] = w.w3;
}

// table [S,16] float32, cdf [S] uint32, tips [T,3] float32: device, the trees' rows concatenated.  tab_off, tip_off, pt_off
// [B+1] int32, seeds [B] uint64, fol_thr [B] uint32, noise, foliage_sigma [B] float32: HOST arrays (they travel as kernel
// arguments, which is what lets the call check them and still be enqueue-only).  Outputs [N,3] / [N], N = pt_off[B], nullable.
extern "C" int st_synth_points_seg(const float* table, const int32_t* tab_off, const uint32_t* cdf, const float* tips,
                                   const int32_t* tip_off, const int32_t* pt_off, int B, const uint64_t* seeds,
                                   const uint32_t* fol_thr, const float* noise, const float* foliage_sigma, float* xyz,
                                   float* medial_vector, float* class_l, int32_t* branch_ids, int32_t* segment, void* stream_) {
    ST_REQUIRE(B >= 0 && B <= SY_MAX_TREES, "synth points: 0 .. %d trees per call (got %d)", SY_MAX_TREES, B);
    if (B == 0) return ST_OK;
    ST_REQUIRE(tab_off && tip_off && pt_off && seeds && fol_thr && noise && foliage_sigma, "synth points: null per-tree array");
    ST_REQUIRE(pt_off[0] == 0, "synth points: pt_off[0] must be 0 (got %d)", (int)pt_off[0]);
    ST_REQUIRE(tab_off[0] >= 0 && tip_off[0] >= 0, "synth points: negative offset (tab_off[0] = %d, tip_off[0] = %d)", (int)tab_off[0],
               (int)tip_off[0]);
    SyTrees T;
    memset(&T, 0, sizeof(T));
    T.n_trees = B;
    T.tab_off[0] = tab_off[0]; T.tip_off[0] = tip_off[0]; T.pt_off[0] = 0;
    for (int s = 0; s < B; s++) {
        ST_REQUIRE(tab_off[s + 1] >= tab_off[s] && tip_off[s + 1] >= tip_off[s] && pt_off[s + 1] >= pt_off[s],
                   "synth points: decreasing offset at tree %d (tab %d -> %d, tip %d -> %d, pt %d -> %d)", s, (int)tab_off[s],
                   (int)tab_off[s + 1], (int)tip_off[s], (int)tip_off[s + 1], (int)pt_off[s], (int)pt_off[s + 1]);
        ST_REQUIRE(pt_off[s + 1] == pt_off[s] || tab_off[s + 1] > tab_off[s], "synth points: tree %d has %d points and no segments", s,
                   (int)(pt_off[s + 1] - pt_off[s]));
        T.tab_off[s + 1] = tab_off[s + 1]; T.tip_off[s + 1] = tip_off[s + 1]; T.pt_off[s + 1] = pt_off[s + 1];
        T.seed_lo[s] = (uint32_t)seeds[s]; T.seed_hi[s] = (uint32_t)(seeds[s] >> 32);
        T.fol_thr[s] = fol_thr[s]; T.noise[s] = noise[s]; T.sigma[s] = foliage_sigma[s];
    }
    const int64_t n = pt_off[B];
    if (n == 0) return ST_OK;
    ST_REQUIRE(table && cdf, "synth points: null segment table");
    ST_REQUIRE(tips || tip_off[B] == tip_off[0], "synth points: null tip list");
    hipLaunchKernelGGL(k_synth_points, dim3((unsigned)st_div_up(n, SY_BLOCK * SY_PPT)), dim3(SY_BLOCK), 0, (hipStream_t)stream_, T, n,
                       (const float4*)table, cdf, tips, xyz, medial_vector, class_l, branch_ids, segment);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
