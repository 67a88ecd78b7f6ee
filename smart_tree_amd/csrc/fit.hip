// st_fit_tubes: fit every tube of a skeleton to the points that were segmented onto it -- one Gauss-Newton step of the geometric
// circle fit per tube, from integer moments that are the same in every run.
//
// The reference has no such step: its radii are the network's per-point prediction carried through the graph (skeleton/path.py),
// corrected by the box filter of `smooth` only.
//
// The contract (tests/fit_oracle.py restates it on its own, on purpose).
// Inputs: pts [n,3]; tube [n] int32, what st_segment_points_seg wrote (a position in the tube arrays, -1: none; a value outside
// [0, m) takes no part); a, b [m,3], r1, r2 [m].
// Frame of a tube (float32, formed once per tube, no contraction): ab = b - a; k = the coordinate with the smallest |ab_k| (strict
//   comparisons from k = 0 on: ties and NaN stay at the lowest); cross(u, w) = (uy*wz - uz*wy, uz*wx - ux*wz, ux*wy - uy*wx);
//   e1 = normalise(cross(ab, unit_k)), e2 = normalise(cross(ab, e1)), normalise(x) = x / sqrtf(dot(x, x)), dot = st_dot3.
// Which points enter: tube in range and the point finite; q = st_tube_num(p) / dot(ab, ab) with 0 <= q <= 1 (false for NaN: a
//   zero-length tube takes no point; a point past an end cap sits on the joint's sphere, not on the cylinder); the pair is
//   st_tube_pair_at(q, ...), rho = sqrtf(d2) and rho > 0; and max_relative < 0 or |res| <= max_relative * r (one float32 product).
// What a point adds: w = (-v) / rho, c = dot(w, e1), s = dot(w, e2); ten int64 sums per tube, moments [m,10]: the count, then
//   fix(c*c), fix(c*s), fix(s*s), fix(c), fix(s), fix(rho*c), fix(rho*s), fix(rho), fix(rho*rho) with
//   fix(x) = llrintf(fminf(fmaxf(x * 2^24, -2^40), 2^40)) (a NaN goes to -2^40: every value has a defined integer).
//   Integer sums: the order of the atomics never shows; |c|, |s| <= 1 and the clamp bound every term by 2^40, so 2^31 points fit.
// The solve, a lane per tube, float64, S* = the sums / 2^24, N = the count: the least squares of rho_i - (c_i, s_i).(cu, cv) - R = 0,
//   normal matrix [[Scc,Scs,Sc],[Scs,Sss,Ss],[Sc,Ss,N]], right side (Src, Srs, Sr), by Cramer's rule.
//   spread = the smaller eigenvalue of [[Scc,Scs],[Scs,Sss]] / N - mean mean^T, mean = (Sc, Ss) / N.
//   status 0 (N < min_points): not fitted, the rest of the row is 0.  status 1 (spread < min_spread, or a full solve that is not
//   finite): R = Sr / N, offset 0.  status 2: (cu, cv, R) of the solve.  rms = sqrt(max(Srr - x.b, 0) / N), x the answer, b the right side.
// Output fit [m,8] float64: N, R, the offset cu*e1 + cv*e2 (three columns), rms, spread, status.
//
// Three kernels: the tube records (pair record and frame), the accumulation, the solve.  The accumulation sums per workgroup in an
// LDS table first (FT_SLOTS tubes, ten int64 each, open addressing): a million points on a few thousand tubes would otherwise queue
// ten global atomics each on as few addresses (segment.hip's tally measured that pattern 250 times slower).  A point whose tube finds
// no slot within FT_PROBES probes adds to global memory itself; every occupied slot is added once at the end.
// Enqueue-only: no allocation, no read-back, no wait.
#include "st_common.h"
#include "st_tube.h"

#define FT_BLOCK 256
#define FT_TILES 8    // points per workgroup = FT_TILES * FT_BLOCK: the table is cleared and flushed once for 2048 points
#define FT_SLOTS 256  // 21 KB of LDS per workgroup: seven workgroups fit a CU's 160 KB
#define FT_PROBES 8
#define FT_MOMENTS 10
#define FT_FIX 16777216.0f
#define FT_CLAMP 1099511627776.0f  // 2^40

struct FtTube {
    float4 A, B;  // st_tube_record's
    float4 E1;    // e1.xyz, dot(ab, ab)
    float4 E2;    // e2.xyz, 0
};

__device__ __forceinline__ void ft_cross(float ux, float uy, float uz, float wx, float wy, float wz, float* o) {
    float p = uy * wz, q = uz * wy;
    o[0] = p - q;
    p = uz * wx; q = ux * wz;
    o[1] = p - q;
    p = ux * wy; q = uy * wx;
    o[2] = p - q;
}
__device__ __forceinline__ void ft_normalise(float* x) {
    const float len = sqrtf(st_dot3(x[0], x[1], x[2], x[0], x[1], x[2]));
    x[0] = x[0] / len; x[1] = x[1] / len; x[2] = x[2] / len;
}
__device__ __forceinline__ unsigned long long ft_fix(float v) {
    return (unsigned long long)llrintf(fminf(fmaxf(v * FT_FIX, -FT_CLAMP), FT_CLAMP));
}

__global__ void __launch_bounds__(FT_BLOCK) k_ft_record(const float* a, const float* b, const float* r1, const float* r2, int64_t m,
                                                        FtTube* rec) {
    const int64_t g = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (g >= m) return;
    FtTube t;
    float ab2;
    st_tube_record(a, b, r1, r2, g, &t.A, &t.B, &ab2, 0);
    int k = 0;
    float least = fabsf(t.B.x);
    if (fabsf(t.B.y) < least) { k = 1; least = fabsf(t.B.y); }
    if (fabsf(t.B.z) < least) k = 2;
    float e1[3], e2[3];
    ft_cross(t.B.x, t.B.y, t.B.z, k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f, e1);
    ft_normalise(e1);
    ft_cross(t.B.x, t.B.y, t.B.z, e1[0], e1[1], e1[2], e2);
    ft_normalise(e2);
    t.E1 = make_float4(e1[0], e1[1], e1[2], ab2);
    t.E2 = make_float4(e2[0], e2[1], e2[2], 0.0f);
    rec[g] = t;
}

// keys [FT_SLOTS], sums [FT_MOMENTS * FT_SLOTS] (moment-major: the lanes of a wave-instruction spread over the slots) are LDS.
__global__ void __launch_bounds__(FT_BLOCK) k_ft_accumulate(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ tube,
                                                            const FtTube* __restrict__ rec, int64_t m, float max_relative,
                                                            unsigned long long* mom) {
    __shared__ int keys[FT_SLOTS];
    __shared__ unsigned long long sums[FT_MOMENTS * FT_SLOTS];
    for (int j = threadIdx.x; j < FT_SLOTS; j += FT_BLOCK) keys[j] = -1;
    for (int j = threadIdx.x; j < FT_MOMENTS * FT_SLOTS; j += FT_BLOCK) sums[j] = 0ull;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (FT_TILES * FT_BLOCK);
    for (int tile = 0; tile < FT_TILES; tile++) {
        const int64_t i = base + (int64_t)tile * FT_BLOCK + threadIdx.x;
        if (i >= n) break;
        const int t = tube[i];
        if (t < 0 || (int64_t)t >= m) continue;
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        if (!(st_finite(px) && st_finite(py) && st_finite(pz))) continue;
        const FtTube T = rec[t];
        const float q = st_tube_num(px, py, pz, T.A, T.B) / T.E1.w;
        if (!(q >= 0.0f && q <= 1.0f)) continue;
        const StPair<float> pr = st_tube_pair_at(q, px, py, pz, T.A, T.B);
        const float rho = sqrtf(pr.d2);
        if (!(rho > 0.0f)) continue;
        if (max_relative >= 0.0f) {
            const float lim = max_relative * pr.r;
            if (!(fabsf(pr.res) <= lim)) continue;
        }
        const float wx = (-pr.vx) / rho, wy = (-pr.vy) / rho, wz = (-pr.vz) / rho;
        const float c = st_dot3(wx, wy, wz, T.E1.x, T.E1.y, T.E1.z), s = st_dot3(wx, wy, wz, T.E2.x, T.E2.y, T.E2.z);
        unsigned long long v[FT_MOMENTS];
        v[0] = 1ull;
        v[1] = ft_fix(c * c); v[2] = ft_fix(c * s); v[3] = ft_fix(s * s);
        v[4] = ft_fix(c); v[5] = ft_fix(s);
        v[6] = ft_fix(rho * c); v[7] = ft_fix(rho * s);
        v[8] = ft_fix(rho); v[9] = ft_fix(rho * rho);
        unsigned slot = ((unsigned)t * 2654435761u) >> 24;  // 8 bits
        bool placed = false;
        for (int probe = 0; probe < FT_PROBES && !placed; probe++, slot = (slot + 1u) & (FT_SLOTS - 1)) {
            const int prev = atomicCAS(&keys[slot], -1, t);
            if (prev == -1 || prev == t) {
#pragma unroll
                for (int k = 0; k < FT_MOMENTS; k++) atomicAdd(&sums[k * FT_SLOTS + slot], v[k]);
                placed = true;
            }
        }
        if (!placed) {  // more tubes in this workgroup's points than the table holds
#pragma unroll
            for (int k = 0; k < FT_MOMENTS; k++) atomicAdd(&mom[FT_MOMENTS * (int64_t)t + k], v[k]);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < FT_SLOTS; j += FT_BLOCK) {
        const int t = keys[j];
        if (t < 0) continue;
#pragma unroll
        for (int k = 0; k < FT_MOMENTS; k++) atomicAdd(&mom[FT_MOMENTS * (int64_t)t + k], sums[k * FT_SLOTS + j]);
    }
}

__global__ void __launch_bounds__(FT_BLOCK) k_ft_solve(const long long* __restrict__ mom, const FtTube* __restrict__ rec, int64_t m,
                                                       int64_t min_points, double min_spread, double* fit) {
    const int64_t g = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (g >= m) return;
    const long long* M = mom + FT_MOMENTS * g;
    double* o = fit + 8 * g;
    const double N = (double)M[0];
    o[0] = N;
    for (int k = 1; k < 8; k++) o[k] = 0.0;
    if (M[0] < min_points || M[0] <= 0) return;
    const double f = 1.0 / 16777216.0;  // (a power of two: the products are exact)
    const double Scc = (double)M[1] * f, Scs = (double)M[2] * f, Sss = (double)M[3] * f, Sc = (double)M[4] * f, Ss = (double)M[5] * f;
    const double Src = (double)M[6] * f, Srs = (double)M[7] * f, Sr = (double)M[8] * f, Srr = (double)M[9] * f;
    const double mc = Sc / N, ms = Ss / N;
    const double cxx = Scc / N - mc * mc, cxy = Scs / N - mc * ms, cyy = Sss / N - ms * ms;
    const double half = 0.5 * (cxx - cyy);
    const double spread = 0.5 * (cxx + cyy) - sqrt(half * half + cxy * cxy);
    double cu = 0.0, cv = 0.0, R = Sr / N, status = 1.0;
    if (spread >= min_spread) {
        // Cramer's rule on the symmetric 3x3
        const double c00 = Sss * N - Ss * Ss, c01 = Ss * Sc - Scs * N, c02 = Scs * Ss - Sss * Sc;
        const double c11 = Scc * N - Sc * Sc, c12 = Scs * Sc - Scc * Ss, c22 = Scc * Sss - Scs * Scs;
        const double det = Scc * c00 + Scs * c01 + Sc * c02;
        const double xu = (c00 * Src + c01 * Srs + c02 * Sr) / det;
        const double xv = (c01 * Src + c11 * Srs + c12 * Sr) / det;
        const double xr = (c02 * Src + c12 * Srs + c22 * Sr) / det;
        if (fabs(xu) <= 1.0e300 && fabs(xv) <= 1.0e300 && fabs(xr) <= 1.0e300) { cu = xu; cv = xv; R = xr; status = 2.0; }
    }
    const double left = Srr - ((cu * Src + cv * Srs) + R * Sr);
    const FtTube T = rec[g];
    o[1] = R;
    if (status == 2.0) {
        o[2] = cu * (double)T.E1.x + cv * (double)T.E2.x;
        o[3] = cu * (double)T.E1.y + cv * (double)T.E2.y;
        o[4] = cu * (double)T.E1.z + cv * (double)T.E2.z;
    }
    o[5] = sqrt((left > 0.0 ? left : 0.0) / N);
    o[6] = spread;
    o[7] = status;
}

// --------------------------------------------------------------------------------------- host ---
struct FtLayout {
    FtTube* rec;
    long long* mom;
};

static void ft_layout(StArena& a, int64_t m, FtLayout* L) {
    L->rec = a.take<FtTube>(m);
    L->mom = a.take<long long>(FT_MOMENTS * m);  // the moments of a caller that does not ask for them
}

static bool ft_sizes_ok(int64_t n, int64_t m) { return n >= 0 && m >= 0 && n < (1ll << 31) && m < (1ll << 31); }

extern "C" int64_t st_fit_tubes_workspace_bytes(int64_t n, int64_t m) {
    if (!ft_sizes_ok(n, m)) return -1;
    StArena a(nullptr, 0);
    FtLayout L;
    ft_layout(a, m, &L);
    return a.used;
}

extern "C" int st_fit_tubes(const float* pts, int64_t n, const int32_t* tube, const float* a, const float* b, const float* r1,
                            const float* r2, int64_t m, float max_relative, int64_t min_points, double min_spread, int64_t* moments,
                            double* fit, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ST_REQUIRE(n >= 0 && n < (1ll << 31), "fit_tubes: 0 <= points < 2^31 (got %lld)", (long long)n);
    ST_REQUIRE(m >= 0 && m < (1ll << 31), "fit_tubes: 0 <= tubes < 2^31 (got %lld)", (long long)m);
    ST_REQUIRE(max_relative == max_relative, "fit_tubes: max_relative is NaN (negative means every point of the tube)");
    ST_REQUIRE(min_spread == min_spread, "fit_tubes: min_spread is NaN");
    ST_REQUIRE(n == 0 || (pts && tube), "fit_tubes: %lld points need their coordinates and their tubes", (long long)n);
    ST_REQUIRE(m == 0 || (a && b && r1 && r2), "fit_tubes: %lld tubes need their end points and radii", (long long)m);
    StArena arena(ws, ws_bytes);
    FtLayout L;
    ft_layout(arena, m, &L);
    if (!arena.ok() || !ws) {
        st_set_error("fit_tubes: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)arena.used);
        return ST_ERR_WORKSPACE;
    }
    if (m == 0) return ST_OK;
    long long* mom = moments ? (long long*)moments : L.mom;
    (void)hipMemsetAsync(mom, 0, (size_t)(FT_MOMENTS * m) * sizeof(long long), stream);
    if (n == 0) {  // no point: every row is (0, ..., status 0)
        if (fit) (void)hipMemsetAsync(fit, 0, (size_t)(8 * m) * sizeof(double), stream);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    const unsigned mb = (unsigned)st_div_up(m, FT_BLOCK);
    hipLaunchKernelGGL(k_ft_record, dim3(mb), dim3(FT_BLOCK), 0, stream, a, b, r1, r2, m, L.rec);
    hipLaunchKernelGGL(k_ft_accumulate, dim3((unsigned)st_div_up(n, FT_TILES * FT_BLOCK)), dim3(FT_BLOCK), 0, stream, pts, n, tube,
                       (const FtTube*)L.rec, m, max_relative, (unsigned long long*)mom);
    if (fit)
        hipLaunchKernelGGL(k_ft_solve, dim3(mb), dim3(FT_BLOCK), 0, stream, (const long long*)mom, (const FtTube*)L.rec, m, min_points,
                           min_spread, fit);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
