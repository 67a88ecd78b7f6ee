// Skeleton evaluation against ground truth: sample a skeleton's tubes at a fixed spacing (st_sample_tubes_*) and match
// every sample to the NEAREST AXIS of another skeleton's tubes with the precision / recall tally fused in (st_skeleton_match).
//
// Replaces  sample_tubes                    smart_tree/data_types/tube.py:53-74  (per tube: arange(0, len, len / n) points,
//                                                                                linspace(r1, r2, count) radii, host loop)
//           TreeSkeleton.sample_skeleton    smart_tree/data_types/tree.py:52-53  (sample_tubes over to_tubes())
//           TreeSkeleton.point_to_skeleton  smart_tree/data_types/tree.py:65-71  (the dense N x M projection of queries.py)
//
// Sampling (the contract; it deviates from the reference on purpose, DESIGN.md "Evaluation"): v = b - a,
//   len = sqrtf((vx*vx + vy*vy) + vz*vz), n = ceil((double)len / spacing), n = 0 for a zero or non-finite len;
//   sample k of n: f = (float)k / (float)n, point a + v*f, radius r1 + (r2 - r1)*f.  Tube i owns [off[i], off[i] + n_i).
// Matching (the pieces and their float32 order are st_tube.h's; tests/eval_oracle.py restates them afresh): per tube, once,
//   inv = 1 / dot(ab,ab) (IEEE division; 0 when dot(ab,ab) == 0, so a zero-length tube is the point a); per pair the reciprocal
//   form of t (a NaN becomes 0), the projection q and d2 = dot(q - p, q - p).  The winner is the first tube with the smallest d2; a
//   NaN or infinite d2 never wins (idx = -1, dist = +inf, tube_rad = NaN when no tube gives a finite d2).
// The pair loop keeps only (d2, t, index): ~30 float32 operations per two pairs on packed multiplies / adds, two LDS
// broadcast reads per tube.  The square root and the radius are taken once per sample after the loop.  COMPUTE-bound.
// Tally: hits with integer atomics (one add per threshold per workgroup), the float64 sums as one partial per workgroup in
// the workspace, added in workgroup order by a second launch -- no float atomics, the tally is a function of the inputs alone.
#include "st_common.h"
#include "st_tube.h"

#define SE_BLOCK 256
#define SE_TILE 512
#define SE_MAX_THR 32
#define SE_SUMS 4

// ------------------------------------------------------------------------------------------------ sampling ---
// Number of samples of one tube (saturated at 2^31: the host refuses such a total) and its axis vector.
__device__ __forceinline__ uint32_t se_tube_samples(const float* __restrict__ a, const float* __restrict__ b, int64_t i, double spacing,
                                                    float& ax, float& ay, float& az, float& vx, float& vy, float& vz) {
    ax = a[3 * i]; ay = a[3 * i + 1]; az = a[3 * i + 2];
    vx = b[3 * i] - ax; vy = b[3 * i + 1] - ay; vz = b[3 * i + 2] - az;
    const float len = sqrtf(st_dot3(vx, vy, vz, vx, vy, vz));
    if (!(len > 0.0f) || !(len <= 3.402823466e+38f)) return 0u;  // zero, NaN or infinite
    const double c = ceil((double)len / spacing);
    return c >= 2147483648.0 ? 0x80000000u : (uint32_t)c;
}

__global__ void __launch_bounds__(SE_BLOCK) k_sample_count(const float* __restrict__ a, const float* __restrict__ b, int64_t m, double spacing,
                                                           uint32_t* __restrict__ count, unsigned long long* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * SE_BLOCK + threadIdx.x;
    float ax, ay, az, vx, vy, vz;
    const uint32_t n = i < m ? se_tube_samples(a, b, i, spacing, ax, ay, az, vx, vy, vz) : 0u;
    if (i < m) count[i] = n;
    unsigned long long s = n;  // 64-bit total: the 32-bit scan would wrap silently
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

__global__ void __launch_bounds__(SE_BLOCK) k_sample_fill(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ r1,
                                                          const float* __restrict__ r2, int64_t m, double spacing,
                                                          const uint32_t* __restrict__ off, int64_t total, float* __restrict__ pts,
                                                          float* __restrict__ rad, int32_t* __restrict__ tube_of) {
    const int64_t s = (int64_t)blockIdx.x * SE_BLOCK + threadIdx.x;
    if (s >= total) return;
    // the last tube whose offset is <= s: empty tubes share their successor's offset, so this is the owner
    int64_t lo = 0, hi = m;  // off[lo] <= s (off[0] = 0), off[hi] > s (hi = m: the total)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= s) lo = mid; else hi = mid;
    }
    float ax, ay, az, vx, vy, vz;
    const uint32_t n = se_tube_samples(a, b, lo, spacing, ax, ay, az, vx, vy, vz);
    const float f = (float)(uint32_t)(s - (int64_t)off[lo]) / (float)n;
    float x = vx * f, y = vy * f, z = vz * f;
    x = ax + x; y = ay + y; z = az + z;
    const float ra = r1[lo];
    float r = (r2[lo] - ra) * f;
    r = ra + r;
    if (pts) { pts[3 * s] = x; pts[3 * s + 1] = y; pts[3 * s + 2] = z; }
    if (rad) rad[s] = r;
    if (tube_of) tube_of[s] = (int32_t)lo;
}

extern "C" int64_t st_sample_tubes_workspace_bytes(int64_t m) {
    StArena a(nullptr, 0);
    a.take<unsigned long long>(1);
    a.take<char>(st_scan_ws_bytes(m));
    return a.used;
}

// a, b [m,3]; count, off [m] int32 out; *total_host = the number of samples (one read-back).
extern "C" int st_sample_tubes_count(const float* a, const float* b, int64_t m, double spacing, int32_t* count, int32_t* off,
                                     int64_t* total_host, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(spacing > 0.0, "sample tubes: spacing must be > 0 (got %g)", spacing);
    ST_REQUIRE(m >= 0 && m < (1ll << 31), "sample tubes: 0 .. 2^31 tubes (got %lld)", (long long)m);
    ST_REQUIRE(total_host != nullptr, "sample tubes: total_host is null");
    *total_host = 0;
    if (m == 0) return ST_OK;
    ST_REQUIRE(a && b && count && off, "sample tubes: null array");
    StArena arena(ws, ws_bytes);
    unsigned long long* total = arena.take<unsigned long long>(1);
    const int64_t scan_bytes = st_scan_ws_bytes(m);
    char* scan_ws = arena.take<char>(scan_bytes);
    if (!arena.ok() || !total || !scan_ws) {
        st_set_error("sample tubes: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    (void)hipMemsetAsync(total, 0, sizeof(unsigned long long), stream);
    hipLaunchKernelGGL(k_sample_count, dim3((unsigned)st_div_up(m, SE_BLOCK)), dim3(SE_BLOCK), 0, stream, a, b, m, spacing,
                       (uint32_t*)count, total);
    ST_TRY(st_exclusive_scan_u32((const uint32_t*)count, (uint32_t*)off, m, nullptr, scan_ws, scan_bytes, stream));
    ST_CHECK_LAUNCH();
    unsigned long long got = 0;
    (void)hipMemcpyAsync(&got, total, sizeof(got), hipMemcpyDeviceToHost, stream);
    st_stream_wait(stream);
    ST_CHECK_LAUNCH();
    ST_REQUIRE(got < (1ull << 31), "sample tubes: %llu samples at spacing %g, the limit is 2^31 - 1: use a larger spacing", got, spacing);
    *total_host = (int64_t)got;
    return ST_OK;
}

// count / off / total as st_sample_tubes_count left them (same a, b, spacing); pts [total,3], rad [total], tube_of [total]
// int32, each nullable.  Enqueue-only.
extern "C" int st_sample_tubes_fill(const float* a, const float* b, const float* r1, const float* r2, int64_t m, double spacing,
                                    const int32_t* off, int64_t total, float* pts, float* rad, int32_t* tube_of, void* stream_) {
    ST_REQUIRE(spacing > 0.0, "sample tubes: spacing must be > 0 (got %g)", spacing);
    ST_REQUIRE(m >= 0 && m < (1ll << 31) && total >= 0 && total < (1ll << 31), "sample tubes: tubes and samples must be below 2^31");
    if (total == 0) return ST_OK;
    ST_REQUIRE(m >= 1 && a && b && r1 && r2 && off, "sample tubes: %lld samples need tubes and their offsets", (long long)total);
    hipLaunchKernelGGL(k_sample_fill, dim3((unsigned)st_div_up(total, SE_BLOCK)), dim3(SE_BLOCK), 0, (hipStream_t)stream_, a, b, r1, r2, m,
                       spacing, (const uint32_t*)off, total, pts, rad, tube_of);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ------------------------------------------------------------------------------------------------ matching ---
__device__ __forceinline__ double se_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void __launch_bounds__(SE_BLOCK) k_skeleton_match(const float* __restrict__ pts, const float* __restrict__ rad, int64_t n,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ r1, const float* __restrict__ r2, int64_t m,
                                                             const float* __restrict__ thr, int n_thr, int ref_mode,
                                                             float* __restrict__ dist, int32_t* __restrict__ idx,
                                                             float* __restrict__ tube_rad, unsigned long long* __restrict__ hits,
                                                             double* __restrict__ partial) {
    // per tube: (a.xyz, 1 / ab.ab), (ab.xyz, r2: not read) -- two LDS reads per tube, the same address in every lane (broadcast)
    __shared__ float4 ta[SE_TILE], tb[SE_TILE];
    __shared__ unsigned s_hits[SE_BLOCK / 64][SE_MAX_THR];
    __shared__ double s_sum[SE_BLOCK / 64][SE_SUMS];
    const int64_t i0 = ((int64_t)blockIdx.x * SE_BLOCK + threadIdx.x) * 2, i1 = i0 + 1;
    const bool live0 = i0 < n, live1 = i1 < n;
    const st_f2 px = {live0 ? pts[3 * i0] : 0.0f, live1 ? pts[3 * i1] : 0.0f};
    const st_f2 py = {live0 ? pts[3 * i0 + 1] : 0.0f, live1 ? pts[3 * i1 + 1] : 0.0f};
    const st_f2 pz = {live0 ? pts[3 * i0 + 2] : 0.0f, live1 ? pts[3 * i1 + 2] : 0.0f};
    const float inf = __uint_as_float(0x7f800000u);
    float bd0 = inf, bd1 = inf, bt0 = 0.0f, bt1 = 0.0f;
    int best0 = -1, best1 = -1;
    st_tube_sweep<SE_BLOCK, SE_TILE>(
        0, m, live0,
        [&](int64_t g, int j) {
            float4 A;
            float ab2;
            st_tube_record(a, b, r1, r2, g, &A, &tb[j], &ab2, 0);
            ta[j] = make_float4(A.x, A.y, A.z, ab2 == 0.0f ? 0.0f : 1.0f / ab2);
        },
        [&](int j, int g) {
            const st_f2 t = st_tube_t_rcp(px, py, pz, ta[j], tb[j], ta[j].w);
            const st_f2 d2 = st_tube_project(t, px, py, pz, ta[j], tb[j]).d2;
            if (d2.x < bd0) { bd0 = d2.x; bt0 = t.x; best0 = g; }  // strict: first minimum; NaN / inf never win
            if (d2.y < bd1) { bd1 = d2.y; bt1 = t.y; best1 = g; }
        });
    // once per sample: distance, the winner's radius at the projection, the tally terms
    const float nan = __uint_as_float(0x7fc00000u);
    const bool ok0 = live0 && best0 >= 0, ok1 = live1 && best1 >= 0;
    const float d0 = sqrtf(bd0), d1 = sqrtf(bd1);
    float tr0 = nan, tr1 = nan;
    if (ok0) tr0 = st_tube_radius(bt0, r1[best0], r2[best0]);
    if (ok1) tr1 = st_tube_radius(bt1, r1[best1], r2[best1]);
    const float rs0 = live0 ? rad[i0] : 0.0f, rs1 = live1 ? rad[i1] : 0.0f;
    const float ref0 = ref_mode ? tr0 : rs0, ref1 = ref_mode ? tr1 : rs1;
    if (live0) { if (dist) dist[i0] = d0; if (idx) idx[i0] = best0; if (tube_rad) tube_rad[i0] = tr0; }
    if (live1) { if (dist) dist[i1] = d1; if (idx) idx[i1] = best1; if (tube_rad) tube_rad[i1] = tr1; }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < n_thr; j++) {  // wave-uniform trip count: every lane of the workgroup reaches the ballots
        const float th = thr[j];
        const float lim0 = th * ref0, lim1 = th * ref1;
        const unsigned c = (unsigned)__popcll(__ballot(ok0 && d0 <= lim0)) + (unsigned)__popcll(__ballot(ok1 && d1 <= lim1));
        if (lane == 0) s_hits[wave][j] = c;
    }
    double acc[SE_SUMS] = {0.0, 0.0, 0.0, 0.0};
    if (ok0) { const float e = fabsf(rs0 - tr0); acc[0] += (double)d0; acc[1] += (double)e; acc[2] += (double)(e / ref0); acc[3] += 1.0; }
    if (ok1) { const float e = fabsf(rs1 - tr1); acc[0] += (double)d1; acc[1] += (double)e; acc[2] += (double)(e / ref1); acc[3] += 1.0; }
#pragma unroll
    for (int k = 0; k < SE_SUMS; k++) {
        const double w = se_wave_sum(acc[k]);
        if (lane == 0) s_sum[wave][k] = w;
    }
    __syncthreads();
    if ((int)threadIdx.x < n_thr) {
        unsigned c = 0;
        for (int w = 0; w < SE_BLOCK / 64; w++) c += s_hits[w][threadIdx.x];
        if (c) atomicAdd(&hits[threadIdx.x], (unsigned long long)c);
    }
    if (threadIdx.x < SE_SUMS) {
        double v = 0.0;
        for (int w = 0; w < SE_BLOCK / 64; w++) v += s_sum[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * SE_SUMS + threadIdx.x] = v;
    }
}

__global__ void k_skeleton_match_sums(const double* __restrict__ partial, int64_t nblocks, double* __restrict__ sums) {
    if (threadIdx.x < SE_SUMS) {
        double v = 0.0;
        for (int64_t blk = 0; blk < nblocks; blk++) v += partial[blk * SE_SUMS + threadIdx.x];  // workgroup order
        sums[threadIdx.x] = v;
    }
}

extern "C" int64_t st_skeleton_match_workspace_bytes(int64_t n) {
    StArena a(nullptr, 0);
    a.take<double>(st_div_up(n > 0 ? n : 1, 2 * SE_BLOCK) * SE_SUMS);
    return a.used;
}

// pts [n,3], rad [n] samples; a, b [m,3], r1, r2 [m] tubes; thr [n_thr] float32 (device); ref_mode 0: tolerance = thr * the
// sample's own radius, 1: thr * the winner's radius at the projection.  dist [n], idx [n] int32, tube_rad [n]: nullable.
// tally (device, 8 * n_thr + 32 bytes): int64 hits[n_thr], then double sums[4] = sum dist, sum |rad - tube_rad|,
// sum |rad - tube_rad| / ref, number of samples with idx >= 0 (only those enter the hits and the sums).  Enqueue-only.
extern "C" int st_skeleton_match(const float* pts, const float* rad, int64_t n, const float* a, const float* b, const float* r1,
                                 const float* r2, int64_t m, const float* thr, int n_thr, int ref_mode, float* dist, int32_t* idx,
                                 float* tube_rad, void* tally, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(m >= 1 && m < (1ll << 31), "skeleton match: 1 .. 2^31 tubes (got %lld)", (long long)m);
    ST_REQUIRE(n >= 0 && n < (1ll << 40), "skeleton match: bad sample count %lld", (long long)n);
    ST_REQUIRE(n_thr >= 1 && n_thr <= SE_MAX_THR, "skeleton match: 1 .. %d thresholds (got %d)", SE_MAX_THR, n_thr);
    ST_REQUIRE(ref_mode == 0 || ref_mode == 1, "skeleton match: ref_mode is 0 (sample radius) or 1 (tube radius), got %d", ref_mode);
    ST_REQUIRE(tally != nullptr && thr != nullptr && a && b && r1 && r2, "skeleton match: null tubes, thresholds or tally");
    (void)hipMemsetAsync(tally, 0, (size_t)n_thr * sizeof(int64_t) + SE_SUMS * sizeof(double), stream);
    if (n == 0) {
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    ST_REQUIRE(pts && rad, "skeleton match: null samples");
    const int64_t nblocks = st_div_up(n, 2 * SE_BLOCK);
    StArena arena(ws, ws_bytes);
    double* partial = arena.take<double>(nblocks * SE_SUMS);
    if (!arena.ok() || !partial) {
        st_set_error("skeleton match: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    unsigned long long* hits = (unsigned long long*)tally;
    double* sums = (double*)((int64_t*)tally + n_thr);
    hipLaunchKernelGGL(k_skeleton_match, dim3((unsigned)nblocks), dim3(SE_BLOCK), 0, stream, pts, rad, n, a, b, r1, r2, m, thr, n_thr,
                       ref_mode, dist, idx, tube_rad, hits, partial);
    hipLaunchKernelGGL(k_skeleton_match_sums, dim3(1), dim3(64), 0, stream, (const double*)partial, nblocks, sums);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
