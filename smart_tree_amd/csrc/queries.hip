// st_points_to_nearest_tube: every point against every tapered tube of a skeleton.
//
// Replaces  pts_to_nearest_tube_gpu   smart_tree/util/queries.py:107-133  (N x M dense torch expression: project on
//           the tube axis with t clipped to [0,1], interpolate the radius, pick the tube minimising |distance - radius|)
//      and  skeleton_to_points        smart_tree/util/queries.py:139-166  (the same in host chunks of 4096 points)
// -- the evaluation utility that labels a cloud with its skeleton.  N x M is 5e9 pairs for a
// 1M-point cloud and a 5000-tube skeleton, so this is the one COMPUTE-bound kernel of the package: a lane owns two
// points (packed float32 adds / multiplies), the tubes stream through LDS in tiles (every lane reads the same tube: LDS broadcast), ~45 float32 operations
// per pair including one IEEE division and one square root.
// The pair expression, its float32 operation order and what a zero-length tube gives are st_tube.h's; here a NaN score counts
// as minimal, as torch.argmin does, and the first minimum wins.  oracle/queries_oracle.py is the independent restatement.
#include "st_common.h"
#include "st_tube.h"

#define QT_BLOCK 256
#define QT_TILE 512

__global__ void __launch_bounds__(QT_BLOCK) k_nearest_tube(const float* __restrict__ pts, int64_t n, const float* __restrict__ a,
                                                           const float* __restrict__ b, const float* __restrict__ r1,
                                                           const float* __restrict__ r2, int64_t m, float* __restrict__ vec,
                                                           int64_t* __restrict__ idx, float* __restrict__ rad) {
    // per tube: (a.xyz, r1), (ab.xyz, r2), ab.ab -- three LDS reads per tube, the same address in every lane (broadcast)
    __shared__ float4 ta[QT_TILE], tb[QT_TILE];
    __shared__ float tab2[QT_TILE];
    const int64_t i0 = ((int64_t)blockIdx.x * QT_BLOCK + threadIdx.x) * 2, i1 = i0 + 1;
    const bool live0 = i0 < n, live1 = i1 < n;
    const st_f2 px = {live0 ? pts[3 * i0] : 0.0f, live1 ? pts[3 * i1] : 0.0f};
    const st_f2 py = {live0 ? pts[3 * i0 + 1] : 0.0f, live1 ? pts[3 * i1 + 1] : 0.0f};
    const st_f2 pz = {live0 ? pts[3 * i0 + 2] : 0.0f, live1 ? pts[3 * i1 + 2] : 0.0f};
    unsigned key0 = 0xffffffffu, key1 = 0xffffffffu;  // 0 = NaN score (minimal), else score bits + 1
    int best0 = 0, best1 = 0;
    float v0x = 0.0f, v0y = 0.0f, v0z = 0.0f, r0 = 0.0f, v1x = 0.0f, v1y = 0.0f, v1z = 0.0f, rr1 = 0.0f;
    st_tube_sweep<QT_BLOCK, QT_TILE>(
        0, m, live0, [&](int64_t g, int j) { st_tube_record(a, b, r1, r2, g, ta, tb, tab2, j); },
        [&](int j, int g) {
            const StPair<st_f2> c = st_tube_pair(px, py, pz, ta[j], tb[j], tab2[j]);
            const unsigned k0 = st_score_key(fabsf(c.res.x)), k1 = st_score_key(fabsf(c.res.y));
            if (k0 < key0) { key0 = k0; best0 = g; v0x = c.vx.x; v0y = c.vy.x; v0z = c.vz.x; r0 = c.r.x; }
            if (k1 < key1) { key1 = k1; best1 = g; v1x = c.vx.y; v1y = c.vy.y; v1z = c.vz.y; rr1 = c.r.y; }
        });
    if (live0) { vec[3 * i0] = v0x; vec[3 * i0 + 1] = v0y; vec[3 * i0 + 2] = v0z; idx[i0] = best0; rad[i0] = r0; }
    if (live1) { vec[3 * i1] = v1x; vec[3 * i1 + 1] = v1y; vec[3 * i1 + 2] = v1z; idx[i1] = best1; rad[i1] = rr1; }
}

// pts [n,3]; a, b [m,3] tube end points, r1, r2 [m] end radii; vec [n,3] (projection - point), idx [n] int64, rad [n].
extern "C" int st_points_to_nearest_tube(const float* pts, int64_t n, const float* a, const float* b, const float* r1,
                                         const float* r2, int64_t m, float* vec, int64_t* idx, float* rad, void* stream_) {
    ST_REQUIRE(m >= 1 && m < (1ll << 31), "nearest tube: the skeleton needs 1 .. 2^31 tubes");
    if (n <= 0) return ST_OK;
    hipLaunchKernelGGL(k_nearest_tube, dim3((unsigned)st_div_up(n, 2 * QT_BLOCK)), dim3(QT_BLOCK), 0, (hipStream_t)stream_, pts, n, a, b,
                       r1, r2, m, vec, idx, rad);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
