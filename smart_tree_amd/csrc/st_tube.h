// A point against a tapered tube: the one definition of the pair expression behind st_points_to_nearest_tube (queries.hip),
// st_segment_points_seg (segment.hip), st_skeleton_match (skeleton_eval.hip) and st_post_process's repair (postprocess.hip).
//
// The contract (float32, this operation order, no contraction; every piece below is the scalar and the packed two-points-per-lane
// form of the same operations, so both give the same bits):
//   ab = b - a;  dot(u, w) = (ux*wx + uy*wy) + uz*wz;  t = clip01(dot(p - a, ab) / dot(ab, ab));  q = a + t*ab
//   r = (1 - t)*r1 + t*r2;  v = q - p;  d2 = dot(v, v);  residual = sqrtf(d2) - r (negative inside the tube);  score = |residual|
// A zero-length tube gives t = 0/0 = NaN and with it a NaN score; what a NaN means is the caller's rule (queries and the repair:
// minimal, as torch.argmin has it -- st_score_key; segment: never wins, and it stages such a tube differently).
// The evaluation's t is different on purpose: dot(p - a, ab) * inv with inv = 1 / dot(ab, ab) taken once per tube (0 for a
// zero-length one) and a clip that sends NaN to 0 -- st_tube_t_rcp; it shares the projection and the radius.
// Each user's oracle (oracle/queries_oracle.py, tests/segment_oracle.py, tests/eval_oracle.py, oracle/pipeline_oracle.py) restates
// this on its own, on purpose.
#pragma once

#include "st_common.h"

typedef float st_f2 __attribute__((ext_vector_type(2)));  // two points per lane: v_pk_{add,mul}_f32 do both at once

template <class T>
__device__ __forceinline__ T st_dot3(T ax, T ay, T az, T bx, T by, T bz) {
    T s = ax * bx;
    T t = ay * by;
    s = s + t;
    t = az * bz;
    return s + t;
}
__device__ __forceinline__ float st_clip01(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }  // NaN stays NaN
__device__ __forceinline__ float st_clip01_nan0(float t) {                                               // NaN -> 0, -0 -> +0
    t = t > 0.0f ? t : 0.0f;
    return t < 1.0f ? t : 1.0f;
}
__device__ __forceinline__ st_f2 st_clip01_nan0(st_f2 t) { return st_f2{st_clip01_nan0(t.x), st_clip01_nan0(t.y)}; }
// clip01(n / d).  The packed form divides and clips one component after the other: written as one packed quotient the same
// instructions come out in another order, and k_nearest_tube measured 1 % slower on an MI355X (profiles/tube_pair_ab.txt).
__device__ __forceinline__ float st_clip01_div(float n, float d) { return st_clip01(n / d); }
__device__ __forceinline__ st_f2 st_clip01_div(st_f2 n, float d) { return st_f2{st_clip01(n.x / d), st_clip01(n.y / d)}; }
__device__ __forceinline__ float st_residual(float d2, float r) { return sqrtf(d2) - r; }
__device__ __forceinline__ st_f2 st_residual(st_f2 d2, st_f2 r) { return st_f2{sqrtf(d2.x) - r.x, sqrtf(d2.y) - r.y}; }
__device__ __forceinline__ bool st_finite(float v) { return fabsf(v) <= 3.4028234e38f; }

// A score >= 0 as the key an unsigned minimum works on: 0 for NaN (minimal), else its bits + 1 (the bits order like the values).
__device__ __forceinline__ unsigned st_score_key(float score) { return score != score ? 0u : __float_as_uint(score) + 1u; }

// The tube as the pair reads it, formed once per tube: A = (a.xyz, r1), B = (ab.xyz, r2), ab2 = dot(ab, ab).
// Written straight to slot j of where it is staged (an LDS tile, a table in memory, three locals with j = 0).  It takes the arrays
// and the slot, not the slots' addresses: formed ahead of the loads, those addresses cost k_nearest_tube its 65th register.
__device__ __forceinline__ void st_tube_record(const float* a, const float* b, const float* r1, const float* r2, int64_t g, float4* ta,
                                               float4* tb, float* tab2, int64_t j) {
    const float ax = a[3 * g], ay = a[3 * g + 1], az = a[3 * g + 2];
    const float dx = b[3 * g] - ax, dy = b[3 * g + 1] - ay, dz = b[3 * g + 2] - az;
    ta[j] = make_float4(ax, ay, az, r1[g]);
    tb[j] = make_float4(dx, dy, dz, r2[g]);
    tab2[j] = st_dot3(dx, dy, dz, dx, dy, dz);
}

// The pieces of the pair, T = float (one point) or st_f2 (two).
template <class T>
__device__ __forceinline__ T st_tube_num(T px, T py, T pz, float4 A, float4 B) {  // dot(p - a, ab)
    return st_dot3<T>(px - A.x, py - A.y, pz - A.z, (T)B.x, (T)B.y, (T)B.z);
}
template <class T>
__device__ __forceinline__ T st_tube_t_div(T px, T py, T pz, float4 A, float4 B, float ab2) {
    return st_clip01_div(st_tube_num(px, py, pz, A, B), ab2);
}
template <class T>
__device__ __forceinline__ T st_tube_t_rcp(T px, T py, T pz, float4 A, float4 B, float inv) {
    return st_clip01_nan0(st_tube_num(px, py, pz, A, B) * inv);
}
template <class T>
__device__ __forceinline__ T st_tube_radius(T t, float r1, float r2) {
    T r = (1.0f - t) * r1;
    const T r_hi = t * r2;
    return r + r_hi;
}
template <class T>
struct StPair {
    T vx, vy, vz, d2, r, res;  // v = projection - point, d2 = dot(v, v); r and res are set by st_tube_pair_at only
};
template <class T>
__device__ __forceinline__ StPair<T> st_tube_project(T t, T px, T py, T pz, float4 A, float4 B) {
    T qx = t * B.x, qy = t * B.y, qz = t * B.z;
    qx = A.x + qx; qy = A.y + qy; qz = A.z + qz;
    StPair<T> o;
    o.vx = qx - px; o.vy = qy - py; o.vz = qz - pz;
    o.d2 = st_dot3(o.vx, o.vy, o.vz, o.vx, o.vy, o.vz);
    return o;
}
// the whole pair from a given t (segment: t = 0 for a zero-length tube) ...
template <class T>
__device__ __forceinline__ StPair<T> st_tube_pair_at(T t, T px, T py, T pz, float4 A, float4 B) {
    const T r = st_tube_radius(t, A.w, B.w);
    StPair<T> o = st_tube_project(t, px, py, pz, A, B);
    o.r = r;
    o.res = st_residual(o.d2, o.r);
    return o;
}
// ... and with t by division
template <class T>
__device__ __forceinline__ StPair<T> st_tube_pair(T px, T py, T pz, float4 A, float4 B, float ab2) {
    return st_tube_pair_at(st_tube_t_div(px, py, pz, A, B, ab2), px, py, pz, A, B);
}

// The sweep of one workgroup over the tubes [begin, end) in LDS tiles of TILE: stage(g, j) puts tube g into slot j, offer(j, g) scores
// slot j (tube g) against the lane's points.  Reached by every lane of the workgroup; a lane that is not live only stages.
template <int BLOCK, int TILE, class Stage, class Offer>
__device__ __forceinline__ void st_tube_sweep(int64_t begin, int64_t end, bool live, Stage stage, Offer offer) {
    for (int64_t base = begin; base < end; base += TILE) {
        const int cnt = (int)(end - base < TILE ? end - base : TILE);
        __syncthreads();  // the previous tile is no longer read
        for (int j = threadIdx.x; j < cnt; j += BLOCK) stage(base + j, j);
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < cnt; j++) offer(j, (int)(base + j));
    }
}
