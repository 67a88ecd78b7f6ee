/* smarttree_hip.h -- C ABI of libsmarttree_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the smart-tree inference hot path.  The reference (uc-vision/smart-tree) has no
 * FFI layer of its own: its heavy arithmetic lives in three CUDA-only third-party packages (spconv, FRNN,
 * cugraph/cudf) that it calls from Python.  Each entry point below replaces one of those call sites; the
 * `replaces:` line cites it (paths relative to the reference's smart_tree/ package).  INTEGRATION.md shows
 * the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (torch tensors) unless its name ends in
 *     `_host`; sizes are explicit; the library never frees or keeps caller memory;
 *   - scratch comes from a caller-provided workspace (`ws`, `ws_bytes`) sized by the matching
 *     `*_workspace_bytes` function (or `st_query_workspace`); no hipMalloc inside the library;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).  Functions that
 *     return a count to the host (`*_host` out-parameters) synchronise that stream once before returning;
 *   - return value: 0 = ok, < 0 = error (-1 invalid argument, -2 workspace too small, -3 HIP error);
 *     `st_last_error()` gives the text (thread local).  Nothing throws.
 *   - neighbour tables are OUTPUT-stationary: nbr[k * n_out + o] = input row or -1, k = (kz*3+ky)*3+kx.
 */
#ifndef SMARTTREE_HIP_H
#define SMARTTREE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101 (round 6): st_abi_entries added; stats_host of the skeleton calls is 16 x int64 (8 before 100) and their tuning array
 * 24 x int64 -- a caller built against an older header must check st_abi_entries before passing shorter arrays.
 * 105: st_centre_cloud_box_seg and st_voxelize_blocks_box_seg added (no existing signature or st_abi_entries value changed);
 * st_component_csr_knn_workspace_bytes asks for one more int32 per table entry.
 * 107: st_synth_points_seg and st_synth_philox added (no existing signature changed).
 * 108: st_prediction_metrics and its three size queries added (no existing signature changed).
 * 109: the st_render_* calls added (no existing signature changed).
 * 110: st_bridge_components_seg and its size query added (no existing signature changed).
 * 111: st_segment_points_seg and its size query added (no existing signature changed).
 * 112: st_brick_pyramid_need, the st_sparse_conv_{mfma,b3,f16}_list_fwd calls, st_pointwise_mlp_heads_keep and st_move_rows_list
 * added; st_abi_entries(3) added (no existing signature or st_abi_entries value changed).
 * 113: st_fit_tubes and its size query added (no existing signature changed).
 * 114: st_tree_tally and its size query added (no existing signature changed).
 * 115: st_ground_extent, st_ground_model, st_ground_height and their size query added (no existing signature changed).
 * 116: the neighbour searches serve a run of queries per wavefront (no signature, workspace size or result changed).
 * 117: st_scan_u32_dev and st_fill_u32_len added for the primitive-level tests; st_sort_pairs_u32 ignores the key bits at and
 * above key_bits (before: it ordered by whole bytes); the coordinate hash probes every slot of a table of up to 4096 slots (no
 * existing signature changed).
 * 118: st_scan_cast_seg and its size query st_scan_cast_workspace_bytes added (no existing signature changed).
 * 119: st_beam_tally_seg and its size query st_beam_tally_workspace_bytes added (no existing signature changed). */
int st_version(void);
/* Array lengths this build of the library reads / writes, so that a caller can check them at run time instead of trusting the
 * header it was compiled against: what = 0 -> int64 entries of `stats_host` (st_skeleton_components*, st_sssp, st_tree_distance,
 * st_sample_tree: all ZEROED and written), 1 -> int64 entries of `tuning` (st_skeleton_components_seg: all READ when non-NULL),
 * 2 -> ST_MAX_SEG (clouds per batched call), 3 -> int64 entries per level of `need_counts_host` (st_brick_pyramid_need: WRITTEN);
 * anything else -> -1 */
#define ST_BRICK_NEED_COUNTS 4
#define ST_SKELETON_STATS_ENTRIES 16
#define ST_SKELETON_TUNING_ENTRIES 24
int st_abi_entries(int what);
const char* st_last_error(void);
/* op: 0 scan(n) 1 sort(n) 2 voxelize(n,max_blocks,max_voxels) 3 strided(n) 4 knn(n_dst) 5 make_edges(n)
 *     6 component_layout(n) 7 component_csr(m) 8 skeleton(m,n_comp) */
int64_t st_query_workspace(int op, int64_t a, int64_t b, int64_t c);

/* ---- primitives (exported for tests) ------------------------------------------------------------ */
int64_t st_scan_workspace_bytes(int64_t n);
int st_scan_u32(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* total, void* ws, int64_t ws_bytes, void* stream);
int64_t st_sort_workspace_bytes(int64_t n);
int st_sort_pairs_u32(uint32_t* keys, uint32_t* vals, int64_t n, int key_bits, void* ws, int64_t ws_bytes, void* stream);
/* the scan over the first min(n, *n_dev) elements (n_dev: device pointer, may be NULL = n); elements past them are neither read
 * nor written, *total = the sum of the live prefix */
int st_scan_u32_dev(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* total, void* ws, int64_t ws_bytes, const int64_t* n_dev,
                    void* stream);
/* p[0 .. min(n, *n_dev)) = value */
int st_fill_u32_len(uint32_t* p, int64_t n, const int64_t* n_dev, uint32_t value, void* stream);

/* ---- blocks + voxelisation ------------------------------------------------------------------------
 * replaces: dataset/dataset.py:166-226 (SingleTreeInference.compute_blocks / __getitem__, i.e.
 *           spconv.pytorch.utils.PointToVoxel.generate_voxel_with_id on the CPU) and model/sparse.py:40-61
 *           (batch_collate).  feats [max_voxels,6], coords [max_voxels,4] (block,z,y,x), mask [max_voxels],
 *           point_index [max_voxels], block_centres [max_blocks,3]. */
int64_t st_voxelize_workspace_bytes(int64_t n_points, int max_blocks, int64_t max_voxels);
int st_voxelize_blocks(const float* xyz, const float* rgb, int64_t n, double voxel_size, double block_size,
                       double buffer_size, int min_points, int max_blocks, int64_t max_voxels, float* feats,
                       int32_t* coords, uint8_t* mask, int64_t* point_index, float* block_centres,
                       int64_t* n_voxels_host, int64_t* n_blocks_host, void* ws, int64_t ws_bytes, void* stream);

/* ---- rulebooks ------------------------------------------------------------------------------------
 * replaces: the indice-pair generation spconv runs inside every SubMConv3d / SparseConv3d /
 *           SparseInverseConv3d forward (model/model_blocks.py:23-35,57-70,90-101,134-143). */
int64_t st_hash_capacity(int64_t n);
int st_build_coord_hash(const int32_t* coords, int64_t n, unsigned long long* keys, unsigned* vals, int64_t cap, void* stream);
int st_build_subm_rulebook(const int32_t* coords, int64_t n, const unsigned long long* keys, const unsigned* vals,
                           int64_t cap, int32_t* nbr /*[27,n]*/, void* stream);
/* (no reference counterpart: spconv orders its voxels by hash) the permutation that sorts the voxels by (batch index,
 * Morton code); running the network on the permuted set and scattering the outputs back gives the same values faster. */
int64_t st_spatial_order_workspace_bytes(int64_t n);
int st_spatial_order(const int32_t* coords, int64_t n, int32_t* order /*[n]*/, void* ws, int64_t ws_bytes, void* stream);
/* rows of `row_words` 32-bit words moved by a permutation: dst[p] = src[order[p]] (scatter = 0) / dst[order[p]] = src[p] */
int st_move_rows(const void* src, int row_words, const int32_t* order, int64_t n, void* dst, int scatter, void* stream);
/* the same move for the n positions list[0 .. n) only (p = list[i]); the other rows of dst are not written */
int st_move_rows_list(const void* src, int row_words, const int32_t* order, const int32_t* list, int64_t n, void* dst, int scatter,
                      void* stream);
int64_t st_strided_workspace_bytes(int64_t n_fine);
int st_build_strided_outputs(const int32_t* coords, int64_t n, int64_t max_out, int32_t* out_coords,
                             unsigned long long* ckeys, unsigned* cvals, int64_t ccap, int64_t* n_out_host,
                             int32_t* extent_host /*[3]*/, void* ws, int64_t ws_bytes, void* stream);
int st_build_strided_rulebook(const int32_t* coords, int64_t n, const unsigned long long* fkeys, const unsigned* fvals,
                              int64_t fcap, const int32_t* out_coords, int64_t n_out, const unsigned long long* ckeys,
                              const unsigned* cvals, int64_t ccap, const int32_t* extent_host,
                              int32_t* nbr_down /*[27,n_out]*/, int32_t* nbr_up /*[27,n]*/,
                              int32_t* up_order /*[n+16] or NULL: fine rows grouped by coordinate parity, entry = row | (8 + class) << 28 (tail = scratch)*/,
                              void* stream);

/* ---- network --------------------------------------------------------------------------------------
 * replaces: spconv's gather-GEMM-scatter conv kernels + torch BatchNorm1d/ReLU/add/cat around them
 *           (model/model_blocks.py:8-243) and, for the heads, SparseFC + F.normalize + exp/argmax
 *           (model_blocks.py:246-285, model/model.py:83-85, model/model_inference.py:87-88).
 * st_sparse_conv_fwd: y = act(bn(sum_k W_k . cat(x0,x1)[nbr[k]]) + residual); w is [K][cin][cout]. */
int st_sparse_conv_fwd(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                       const float* w, int cout, const float* scale, const float* shift, const float* residual,
                       int relu, float* y, const int32_t* row_order /*[n_out] or NULL: launch order of the output rows (bits 0-27 row, top 4 bits 0 or the parity tag of st_build_strided_rulebook)*/,
                       void* stream, int64_t nbr_stride /*elements between the rows of nbr; 0 = n_out*/);
/* same contract; weights pre-permuted to wp[K][cin/16][4][cout][4] = W[k][16c+4kg+s][co]; cin, cout, c0 % 16 == 0.
 * The per-offset [16 x cin].[cin x cout] contraction runs on v_mfma_f32_16x16x4_f32 (exact fp32). */
int st_sparse_conv_mfma_fwd(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                            const float* wp, int cout, const float* scale, const float* shift, const float* residual,
                            int relu, float* y, const int32_t* row_order /*[n_out] or NULL: launch order of the output rows (bits 0-27 row, top 4 bits 0 or the parity tag of st_build_strided_rulebook)*/,
                            void* stream, int64_t nbr_stride /*0 = n_out*/,
                            int variant /*0 = the library picks the tile shape by size;
 else row tiles per wave | (weights through LDS) << 4 (bench aid)*/);
/* The same contraction on the bf16 matrix pipe at float32 accuracy: every float32 operand is cut into three bf16 pieces that sum
 * to it exactly and six of the nine piece products are issued (csrc/sparse_conv.hip "split-bf16 rule-GEMM").  Features stay float32;
 * wq = the weights as three bf16 planes in operand order [K][Cin/32][3][4][Cout][8] (smart_tree_amd/model/sparse_ops.py b3_weight).
 * Cin % 32 == 0, Cout % 16 == 0, c0 % 8 == 0.  variant: 0 = row tiles per wavefront by size, 1 / 2 = forced.
 * replaces: the same spconv calls as st_sparse_conv_fwd (model_blocks.py:57-70,90-101,134-143) on the 32- and 64-channel levels */
int st_sparse_conv_b3_fwd(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out, const void* wq,
                          int cout, const float* scale, const float* shift, const float* residual, int relu, float* y,
                          const int32_t* row_order, void* stream, int64_t nbr_stride, int variant);
/* Half-precision storage (BASELINE.json configs[4]; an extension -- the reference's inference, model/model_inference.py:49-100,
 * is float32): in_half && out_half -> x0 / x1 / residual / y are IEEE half, Cin, Cout and the concat split multiples of 16,
 * matrix cores with float32 accumulation; exactly one of them -> the float32 kernel with a converting load or store
 * (w [K][cin][cout] float32, no residual, no concat).
 * WEIGHT LAYOUT of the in_half && out_half form (half elements; smart_tree_amd/model/sparse_ops.py mfma_weight16_half builds it)
 * depends on the channel counts -- a buffer in another order gives wrong results, the call cannot tell:
 *   Cin % 32 == 0                      wp[K][Cin/32][4][Cout][8]      = W[k][32c + 8g + e][co]   (v_mfma_f32_16x16x32_f16)
 *   Cin == 16 and Cout in {16, 32}     pairs of kernel offsets stacked into 32-channel chunks: W' = W padded with a zero offset to
 *                                      an even K, viewed as [K/2][32][Cout], then the order above (K/2 chunks of 32 channels)
 * st_sparse_conv_b3_fwd's wq follows the first two rules with three bf16 planes per chunk ([..][3][4][Cout][8]): Cin == 16 uses
 * the stacked-pair chunks as well (sparse_ops.py b3_weight). */
int st_sparse_conv_f16_fwd(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                           const void* w, int cout, const float* scale, const float* shift, const void* residual, int relu,
                           void* y, int in_half, int out_half, const int32_t* row_order, void* stream, int64_t nbr_stride /*0 = n_out*/);
/* The three matrix-core calls over a LIST of the level's rows (no reference counterpart: the reference evaluates every halo voxel and
 * throws the result away, model/model_inference.py:97-100).  row_order [n_out] names the rows to compute, y has level_rows rows and
 * the others are not written.  The kernel instance and row-tile variant are the ones the plain call picks for n_out = level_rows
 * with (parity != 0) or without a parity order -- never a function of the list -- so a row has the same bits in a list launch and in
 * a launch of the whole level.  parity != 0: the list is a sub-list of the tagged parity order.  (st_sparse_conv_fwd has one kernel
 * per shape at every size: it takes a list as its row_order.) */
int st_sparse_conv_mfma_list_fwd(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                 const float* wp, int cout, const float* scale, const float* shift, const float* residual, int relu,
                                 float* y, const int32_t* row_order, void* stream, int64_t nbr_stride, int variant, int64_t level_rows,
                                 int parity);
int st_sparse_conv_b3_list_fwd(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out, const void* wq,
                               int cout, const float* scale, const float* shift, const float* residual, int relu, float* y,
                               const int32_t* row_order, void* stream, int64_t nbr_stride, int variant, int64_t level_rows, int parity);
int st_sparse_conv_f16_list_fwd(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                                const void* w, int cout, const float* scale, const float* shift, const void* residual, int relu,
                                void* y, int in_half, int out_half, const int32_t* row_order, void* stream, int64_t nbr_stride,
                                int64_t level_rows, int parity);

/* ---- rulebooks without hash probes (csrc/brick.hip) ------------------------------------------------
 * replaces, for the network's own forward pass, the per-conv hash build of spconv (model/model_blocks.py:57-70,90-101,134-143)
 * AND the builders above: every level's active set is kept as 8 x 8 x 8 occupancy bricks with popcount ranks, the voxels of a
 * level are ordered (block, brick Morton code, z, y, x), a neighbour look-up is a table entry + one mask word.  One call builds
 * every level (sets, submanifold tables, strided / inverse tables, parity order) with the counts on the device and ONE
 * read-back.  Tables are laid out with row stride caps[level] (pass it as nbr_stride to the convolutions).
 * st_brick_pyramid_workspace_bytes returns 0 when the structure cannot be sized for the arguments (use the builders above). */
int64_t st_brick_pyramid_workspace_bytes(int64_t n0, int n_blocks, int coord_bound, int depth, const int64_t* caps);
int st_brick_pyramid(const int32_t* coords0 /*[n0,4] (batch index, z, y, x), any order*/, int64_t n0, int n_blocks /*batch indices < this*/,
                     int coord_bound /*z, y, x < this*/, int depth, const int32_t* blk_seg /*[n_blocks] cloud of a batch index or NULL*/,
                     int nseg, const int64_t* caps /*[depth+1] row capacity per level, caps[0] >= n0*/,
                     int32_t* order0 /*[n0]: row p of level 0 = input voxel order0[p]*/, int32_t* const* coords_out /*[depth+1] x [caps[l],4]*/,
                     int32_t* const* subm /*[depth+1] x [27][caps[l]]*/, int32_t* const* down /*[depth] x [27][caps[l+1]]*/,
                     int32_t* const* up /*[depth] x [27][caps[l]]*/, int32_t* const* up_order /*[depth] x [caps[l] + 16]*/,
                     int64_t* counts_host /*[depth+1] rows per level*/, void* ws, int64_t ws_bytes, void* stream);
/* st_brick_pyramid plus the rows the decoder needs when only the INNER voxels' outputs are kept (blocks with a halo; the rule and its
 * thresholds a[l] = 0, 1, 2, 2, ...: csrc/st_rule.h).  inner [n0] uint8 in input order, 1 = kept (NULL: no lists, = st_brick_pyramid).
 * Per level l < depth: need_order[l] = the level's rows with margin <= a[l], then = a[l] + 1, then = a[l] + 2 (brick order inside
 * each part); up_need[l] = the entries of up_order[l] whose row has margin <= a[l] + 2, tags and parity grouping kept;
 * need_counts_host[ST_BRICK_NEED_COUNTS * l + 0 .. 2] = the three prefix lengths of need_order[l], [+ 3] = the length of up_need[l].
 * The counts ride on the call's one read-back.  Same workspace as st_brick_pyramid. */
int st_brick_pyramid_need(const int32_t* coords0, int64_t n0, int n_blocks, int coord_bound, int depth, const int32_t* blk_seg, int nseg,
                          const int64_t* caps, int32_t* order0, int32_t* const* coords_out, int32_t* const* subm, int32_t* const* down,
                          int32_t* const* up, int32_t* const* up_order, int64_t* counts_host, const unsigned char* inner /*[n0] or NULL*/,
                          int32_t* const* need_order /*[depth] x [caps[l]]*/, int32_t* const* up_need /*[depth] x [caps[l]]*/,
                          int64_t* need_counts_host /*[ST_BRICK_NEED_COUNTS * depth]*/, void* ws, int64_t ws_bytes, void* stream);
int st_head_param_floats(void);
int st_pointwise_mlp_heads(const float* x, int64_t n, const float* params, float* radius, float* direction,
                           float* class_l, float* medial_vector /*nullable*/, int64_t* class_idx /*nullable*/, void* stream);
/* the heads of the rows with keep[i] != 0 only (keep [n] uint8; NULL: every row): the other rows of x are not read, their outputs are zero */
int st_pointwise_mlp_heads_keep(const float* x, int64_t n, const unsigned char* keep, const float* params, float* radius, float* direction,
                                float* class_l, float* medial_vector /*nullable*/, int64_t* class_idx /*nullable*/, void* stream);

/* ---- skeleton stage -------------------------------------------------------------------------------
 * st_medial_points  replaces: Cloud.medial_pts / Cloud.radius, data_types/cloud.py:229-231,254-256
 * st_knn_radius     replaces: frnn.frnn_grid_points via skeleton/graph.py:12-33 (filter.py:7, graph.py:37, path.py:30)
 * st_make_edges     replaces: skeleton/graph.py:52-60
 * st_connected_components / st_component_layout / st_component_csr
 *                   replace: cugraph.connected_components + subgraph + the cudf->pandas->torch renumbering,
 *                            data_types/graph.py:32-66, skeleton/skeletonize.py:60-71, skeleton/graph.py:80-104
 * st_skeleton_components (stages 1|2|4) and its single-stage forms st_sssp / st_tree_distance / st_sample_tree
 *                   replace: cugraph.sssp (skeleton/shortest_path.py:12-21), pred_graph + second sssp
 *                            (shortest_path.py:46-55, skeletonize.py:80-85), sample_tree (skeleton/path.py:9-140)
 * st_assemble_branches replaces: the BranchSkeleton / TreeSkeleton construction of skeleton/path.py:128-140 and
 *                   skeletonize.py:86-95 (flat layout consumed by st_post_process)
 * st_post_process   replaces: pipeline.py:95-106 over data_types/tree.py:73-134,164-176 (+ util/queries.py:89-133).
 *                   Branch tables as st_assemble_branches lays them out: a parent has a smaller id than its children (the
 *                   reference's dict walk relies on the same order), every branch owns at least two rad_out slots (they
 *                   carry a key between the call's launches before the radii are written). */
/* st_centre_cloud replaces: dataset/augmentations.py:38-41 (CentreCloud over Cloud.bbox, data_types/cloud.py:222-227) */
int st_centre_cloud(const float* xyz, int64_t n, float* out, void* ws, int64_t ws_bytes, void* stream);
int st_medial_points(const float* xyz, const float* mv, int64_t n, float* medial, float* radius, void* stream);
int64_t st_knn_workspace_bytes(int64_t n_dst);
/* r < 0 (with a bound array): the search radius is max(bound[0..n1)), reduced on the device -- the callers
 * (skeleton/filter.py, skeleton/graph.py) no longer read it back just to pass it in; cell_hint < 0: cell = max(r / -cell_hint, 1e-4).
 * K = 1, 8, 16 or 32 (the rows come out sorted by (distance, index): any other K <= 32 is the first K columns of the next width).
 * NaN / infinite points are nobody's neighbour and find none; a NaN bound admits nobody, an infinite one every point within r. */
int st_knn_radius(const float* src, int64_t n1, const float* dst, int64_t n2, int K, float r, const float* bound,
                  int bound_mode, float cell_hint, int64_t* idx, float* dist, void* ws, int64_t ws_bytes, void* stream);
int64_t st_make_edges_workspace_bytes(int64_t n);
/* n_edges_host may be NULL: the edge count stays on the device and the tail of edges / w [n*K] is padded with (0, 0)
 * self loops of weight 0, which the component entry points below ignore (real edges have dst > 0) */
int st_make_edges(const int64_t* idx, const float* dist, int64_t n, int K, int64_t* edges, float* w,
                  int64_t* n_edges_host, void* ws, int64_t ws_bytes, void* stream);
int64_t st_connected_components_workspace_bytes(int64_t n);
int st_connected_components(const int64_t* edges, int64_t E, int64_t n, int32_t* labels, void* ws, int64_t ws_bytes, void* stream);
int64_t st_component_layout_workspace_bytes(int64_t n);
int st_component_layout(const int32_t* labels, int64_t n, int min_vertices, int32_t* comp_size, int32_t* comp_off,
                        int32_t* vert_order, int32_t* new_id, int64_t* n_comp_host, int64_t* n_kept_host, void* ws,
                        int64_t ws_bytes, void* stream);
int64_t st_component_csr_workspace_bytes(int64_t m);
int st_component_csr(const int64_t* edges, const float* w, int64_t E, const int32_t* new_id, int64_t m, uint32_t* row_off,
                     uint32_t* col, float* wgt, void* ws, int64_t ws_bytes, void* stream);
int64_t st_skeleton_workspace_bytes(int64_t m, int64_t n_comp);
/* stats_host: optional, 16 x int64 (see csrc/skeleton.hip): [0] SSSP rounds .. [6] = branches of the cloud | path vertices << 32
 * (sample_tree stage), [7] in: time the select launches, [8] helper workgroups were lost (fall-back ran), [9] helper workgroups launched,
 * [10] form of the SSSP that produced dist: 0 a launch per round, 1 the persistent launch completed, 2 it gave up at a barrier and
 * the rounds were redone by launches.
 * comp_size_host is unused and may be NULL (the claim grid is laid out on the device from comp_off); grid_cell < 0:
 * cell = max(max(rad) / -grid_cell, 1e-4) with the maximum reduced on the device -- neither costs the caller a read-back */
int st_skeleton_components(int n_comp, const int32_t* comp_off, const int32_t* comp_size_host, int64_t m, const float* pts,
                           const float* rad, const float* ysurf, const uint32_t* row_off, const uint32_t* col,
                           const float* wgt, float grid_cell, int stages, int block_threads, float* dist, int32_t* pred,
                           int32_t* root_local, float* tree_dist, int32_t* branch_parent, int32_t* branch_off,
                           int32_t* branch_len, int32_t* n_branches, int32_t* path_verts, int32_t* branch_of,
                           int64_t* stats_host, void* ws, int64_t ws_bytes, void* stream);
#define ST_SKELETON_STAGE_ARGS                                                                                          \
    int n_comp, const int32_t *comp_off, const int32_t *comp_size_host, int64_t m, const float *pts, const float *rad, \
        const float *ysurf, const uint32_t *row_off, const uint32_t *col, const float *wgt, float grid_cell,           \
        int block_threads, float *dist, int32_t *pred, int32_t *root_local, float *tree_dist, int32_t *branch_parent,  \
        int32_t *branch_off, int32_t *branch_len, int32_t *n_branches, int32_t *path_verts, int32_t *branch_of,        \
        int64_t *stats_host, void *ws, int64_t ws_bytes, void *stream
int st_sssp(ST_SKELETON_STAGE_ARGS);
int st_tree_distance(ST_SKELETON_STAGE_ARGS);
int st_sample_tree(ST_SKELETON_STAGE_ARGS);
int64_t st_assemble_workspace_bytes(int64_t cap_b);
/* counts_host may be NULL: no read-back; the caller takes branches B = stats_host[6] & 0xffffffff and geometry slots
 * P = (stats_host[6] >> 32) + B from st_skeleton_components (totals carried by its last progress read-back).
 * Capacities: parent / start / length are cap_b long, xyz / rad cap_p.  When B > cap_b or P > cap_p nothing outside them is
 * read or written: the first min(B, cap_b) branches are laid out (start [cap_b] is always filled), of their geometry the
 * first cap_p slots, and tree_off [n_comp + 1] is complete.  With counts_host the call then returns ST_ERR_INVALID and
 * counts_host holds the B and P that were needed; with NULL it returns ST_OK -- the caller vouches for the capacities, or
 * compares tree_off[n_comp] with cap_b itself. */
int st_assemble_branches(int n_comp, const int32_t* comp_off, const int32_t* n_branches, const int32_t* branch_parent,
                         const int32_t* branch_off, const int32_t* branch_len, const int32_t* path_verts,
                         const int32_t* vert_order, const float* medial, const float* radius, int32_t* tree_off,
                         int32_t* parent, int32_t* start, int32_t* length, float* xyz, float* rad, int64_t cap_b,
                         int64_t cap_p, int64_t* counts_host, void* ws, int64_t ws_bytes, void* stream);
int st_post_process(int n_trees, const int32_t* tree_off, const int32_t* parent, const int32_t* start, const int32_t* len,
                    float* xyz, const float* rad_in, float* rad_out, uint8_t* keep, uint8_t* repaired, uint8_t* smoothed,
                    int32_t* depth_scratch, int do_prune, float min_radius, float min_length, int do_repair, int do_smooth, int kernel_size,
                    void* stream);

/* st_points_to_nearest_tube replaces: pts_to_nearest_tube_gpu (util/queries.py:107-133) and the chunk loop of
 * skeleton_to_points (util/queries.py:139-166): per point the tube minimising |distance - interpolated radius|. */
int st_points_to_nearest_tube(const float* pts, int64_t n, const float* a, const float* b, const float* r1, const float* r2,
                              int64_t m, float* vec, int64_t* idx, float* rad, void* stream);

/* ---- skeleton evaluation against ground truth (csrc/skeleton_eval.hip) ---------------------------------
 * replaces: sample_tubes (data_types/tube.py:53-74): per tube arange(0, len, len / n) points with linspace radii, a host loop
 * replaces: TreeSkeleton.sample_skeleton (data_types/tree.py:52-53): sample_tubes over to_tubes()
 * replaces: TreeSkeleton.point_to_skeleton (data_types/tree.py:65-71): the dense N x M projection, here by NEAREST AXIS
 * Tubes are (a, b [m,3]; r1, r2 [m]) float32 in to_tubes() order.
 * Sampling: len = sqrtf(dot(v, v)), v = b - a; n = ceil((double)len / spacing), 0 for a zero or non-finite length; sample
 * k < n is a + v * f with radius r1 + (r2 - r1) * f, f = (float)k / (float)n; tube i owns samples [off[i], off[i] + n_i).
 * st_sample_tubes_count writes n and the exclusive offsets (int32 [m] each) and reads the total back (refused from 2^31);
 * st_sample_tubes_fill (enqueue-only) writes pts [total,3], rad [total], tube_of [total] int32, each nullable.
 * Matching: t = clip01(dot(ap, ab) * (1 / dot(ab, ab))), a zero-length tube is the point a; d2 = |a + t ab - p|^2; the
 * first tube with the smallest finite d2 wins (none: idx = -1, dist = +inf, tube_rad = NaN).  Per sample, nullable:
 * dist = sqrtf(d2), idx (int32), tube_rad = (1 - t) r1 + t r2.  tally (device, 8 * n_thr + 32 bytes): int64 hits[n_thr]
 * = samples with idx >= 0 and dist <= thr[j] * ref (ref_mode 0: the sample's rad, 1: the winner's tube_rad), then double
 * sums[4] = sum dist, sum |rad - tube_rad|, sum |rad - tube_rad| / ref, number of samples with idx >= 0.  The tally is
 * bit-identical from run to run (integer atomics; float64 partials per workgroup added in workgroup order).  1 <= n_thr <= 32;
 * thr is a device array.  Enqueue-only; n == 0 zeroes the tally. */
int64_t st_sample_tubes_workspace_bytes(int64_t m);
int st_sample_tubes_count(const float* a, const float* b, int64_t m, double spacing, int32_t* count, int32_t* off,
                          int64_t* total_host, void* ws, int64_t ws_bytes, void* stream);
int st_sample_tubes_fill(const float* a, const float* b, const float* r1, const float* r2, int64_t m, double spacing,
                         const int32_t* off, int64_t total, float* pts, float* rad, int32_t* tube_of, void* stream);
int64_t st_skeleton_match_workspace_bytes(int64_t n);
int st_skeleton_match(const float* pts, const float* rad, int64_t n, const float* a, const float* b, const float* r1,
                      const float* r2, int64_t m, const float* thr, int n_thr, int ref_mode, float* dist, int32_t* idx,
                      float* tube_rad, void* tally, void* ws, int64_t ws_bytes, void* stream);

/* ---- batched forms: B independent clouds in ONE launch set -------------------------------------------
 * replaces: the batch dimension of the reference's data path -- model/sparse.py:40-61 (batch_collate writes the
 *           sample index into coords[:,0]) and model/model_inference.py:62-78 (one forward per collated batch) --
 *           extended over the whole of Pipeline.process_cloud (pipeline.py:55-93), which the reference runs one
 *           cloud at a time.  Cloud s of a batch owns the index range [seg_off[s], seg_off[s+1]) of the batched
 *           arrays (seg_off: device int32 [nseg+1], nseg <= 64).  Every function returns, for every cloud, exactly
 *           what its one-cloud form returns for that cloud alone (indices are positions in the batched arrays):
 *           clouds never share a neighbourhood, a grid slab, a spatial extent or a component. */
int st_centre_cloud_seg(const float* xyz, int64_t n, const int32_t* seg_off, int nseg, float* out, void* ws,
                        int64_t ws_bytes /* >= 24 * nseg + 256 */, void* stream);
/* st_centre_cloud_box_seg = st_centre_cloud_seg that also leaves, per cloud, the bounding box of the CENTRED points in box_out
 * (device, [nseg][6] float: min xyz, max xyz; min = +inf, max = -inf for an empty cloud).  st_voxelize_blocks_box_seg =
 * st_voxelize_blocks_seg that takes that box (centred_box, NULL = none) instead of reducing it from the points once more: valid
 * only for the very array the centring call wrote (same points, same seg_off).  Results are identical with and without it. */
int st_centre_cloud_box_seg(const float* xyz, int64_t n, const int32_t* seg_off, int nseg, float* out, void* ws,
                            int64_t ws_bytes /* >= 24 * nseg + 256 */, void* stream, float* box_out);
int st_voxelize_blocks_box_seg(const float* xyz, const float* rgb, int64_t n, const int32_t* seg_off, int nseg,
                               double voxel_size, double block_size, double buffer_size, int min_points, int max_blocks,
                               int64_t max_voxels, float* feats, int32_t* coords, uint8_t* mask, int64_t* point_index,
                               float* block_centres, int32_t* blk_seg, int32_t* seg_vox_off, int32_t* seg_blk_off,
                               int64_t* n_voxels_host, int64_t* n_blocks_host, void* ws, int64_t ws_bytes, void* stream,
                               const float* centred_box /*[nseg][6] or NULL*/);
int64_t st_voxelize_workspace_bytes_seg(int64_t n_points, int max_blocks, int64_t max_voxels, int nseg);
int st_voxelize_blocks_seg(const float* xyz, const float* rgb, int64_t n, const int32_t* seg_off, int nseg,
                           double voxel_size, double block_size, double buffer_size, int min_points, int max_blocks,
                           int64_t max_voxels, float* feats, int32_t* coords, uint8_t* mask, int64_t* point_index,
                           float* block_centres, int32_t* blk_seg /*[max_blocks] cloud of every block*/,
                           int32_t* seg_vox_off /*[nseg+1]*/, int32_t* seg_blk_off /*[nseg+1]*/, int64_t* n_voxels_host,
                           int64_t* n_blocks_host, void* ws, int64_t ws_bytes, void* stream);
int st_build_strided_outputs_seg(const int32_t* coords, int64_t n, int64_t max_out, int32_t* out_coords,
                                 unsigned long long* ckeys, unsigned* cvals, int64_t ccap, int64_t* n_out_host,
                                 int32_t* extent_host, const int32_t* blk_seg, int nseg, int32_t* ext_dev /*[nseg*3] out*/,
                                 void* ws, int64_t ws_bytes, void* stream);
int st_build_strided_rulebook_seg(const int32_t* coords, int64_t n, const unsigned long long* fkeys, const unsigned* fvals,
                                  int64_t fcap, const int32_t* out_coords, int64_t n_out, const unsigned long long* ckeys,
                                  const unsigned* cvals, int64_t ccap, const int32_t* extent_host, int32_t* nbr_down,
                                  int32_t* nbr_up, int32_t* up_order, const int32_t* blk_seg, const int32_t* ext_dev,
                                  void* stream);
/* Whole-cloud voxelisation of `nseg` clouds (the training / evaluation data path).
 * replaces: TreeDataset.process_cloud's PointToVoxel call (smart_tree/dataset/dataset.py:103-131: range = the cloud's own
 *           bounding box, one point per voxel) + batch_collate's batch column (model/sparse.py:40-61).
 * coords [M,4] = (cloud, z, y, x); feats [M,6] = xyz, rgb of the representative point; point_index [M] = its position in the
 * input (gather any other per-point feature with it); mask [M] = 1 (loss_mask); seg_vox_off [nseg+1] device, may be null for
 * one cloud.  Voxels come out cloud by cloud in order of first appearance. */
int64_t st_voxelize_cloud_workspace_bytes(int64_t n_points, int64_t max_voxels, int nseg);
int st_voxelize_cloud_seg(const float* xyz, const float* rgb, int64_t n, const int32_t* seg_off, int nseg, double voxel_size,
                          int64_t max_voxels, float* feats, int32_t* coords, uint8_t* mask, int64_t* point_index,
                          int32_t* seg_vox_off, int64_t* n_voxels_host, void* ws, int64_t ws_bytes, void* stream);
int64_t st_knn_workspace_bytes_seg(int64_t n_dst, int nseg);
/* cell_mean_mult (with cell_hint < 0): the grid cell is at most this multiple of the MEAN per-query bound (< 0: library
 * default, 0: no cap); it changes the speed of a search, never its result (test hook, tests/test_skeleton.py) */
int st_knn_radius_seg(const float* src, int64_t n1, const float* dst, int64_t n2, int K, float r, const float* bound,
                      int bound_mode, float cell_hint, int64_t* idx, float* dist, const int32_t* src_seg_off,
                      const int32_t* dst_seg_off, int nseg, void* ws, int64_t ws_bytes, void* stream, float cell_mean_mult);
/* replaces: skeleton/filter.py:6-11 (outlier_removal): mask[i] = the query has >= K neighbours inside its bound, i.e.
 *           st_knn_radius_seg(...).idx[:, K-1] != -1 without the neighbour lists (K = 8; workspace as st_knn_radius_seg). */
int st_radius_count_seg(const float* src, int64_t n1, const float* dst, int64_t n2, int K, float r, const float* bound,
                        int bound_mode, float cell_hint, uint8_t* mask, const int32_t* src_seg_off,
                        const int32_t* dst_seg_off, int nseg, void* ws, int64_t ws_bytes, void* stream, float cell_mean_mult,
                        const uint8_t* valid /* optional [n1], needs src == dst: the search runs over the points with valid[i] != 0 only
                        (neighbours and queries alike; mask = 0 for the others) -- the class filter folded into outlier_removal
                        without compacting the cloud in between */);
/* components / adjacency straight from the neighbour search (idx / dist [n,K] of st_knn_radius_seg after the caller's radius
 * filter): the edge set is make_edges' (graph.py:52-60: (i, idx) for idx > vertex 0 of i's cloud) without materialising
 * the int64 edge list.  Same labels as st_connected_components on st_make_edges_seg's output; the CSR holds the same
 * (neighbour, weight) pairs per row as st_component_csr's, but every pair ONCE: a mutual pair (v in kNN(u), u in kNN(v)) is two
 * edges of the list and two entries per row there, one here (the reference's cugraph graph is undirected, one edge per pair).
 * Row layout: valid forward neighbours in table order, then the reverse-only ones.  With a workspace smaller than
 * st_component_csr_knn_workspace_bytes (st_component_csr_workspace_bytes is the minimum) or a K that is not a power of two
 * <= 64 the call builds st_component_csr's rows. */
int64_t st_component_csr_knn_workspace_bytes(int64_t m, int64_t n, int K);
int st_connected_components_knn(const int64_t* idx, int64_t n, int K, const int32_t* first_of /*[n] first vertex of the
                                vertex's cloud; NULL = one cloud*/, int32_t* labels, void* ws, int64_t ws_bytes, void* stream);
int st_component_csr_knn(const int64_t* idx, const float* dist, int64_t n, int K, const int32_t* first_of,
                         const int32_t* new_id, int64_t m, uint32_t* row_off, uint32_t* col, float* wgt, void* ws,
                         int64_t ws_bytes, void* stream);
int st_make_edges_seg(const int64_t* idx, const float* dist, int64_t n, int K, int64_t* edges, float* w,
                      int64_t* n_edges_host, const int32_t* seg_off, int nseg, void* ws, int64_t ws_bytes, void* stream);
int st_component_layout_seg(const int32_t* labels, int64_t n, int min_vertices, const int32_t* seg_off, int nseg,
                            int32_t* comp_size, int32_t* comp_off, int32_t* vert_order, int32_t* new_id,
                            int32_t* comp_seg /*[C]*/, int32_t* comp_seg_off /*[nseg+1]*/, int32_t* vert_seg_off /*[nseg+1]*/,
                            int64_t* n_comp_host, int64_t* n_kept_host, void* ws, int64_t ws_bytes, void* stream,
                            int64_t* max_comp_host /*optional: vertices of the largest kept component (same read-back)*/);
int64_t st_skeleton_workspace_bytes_seg(int64_t m, int64_t n_comp, int nseg);
int st_skeleton_components_seg(int n_comp, const int32_t* comp_off, const int32_t* comp_seg, const int32_t* vert_seg_off,
                               int nseg, int64_t m, const float* pts, const float* rad, const float* ysurf,
                               const uint32_t* row_off, const uint32_t* col, const float* wgt, float grid_cell, int stages,
                               int block_threads, float* dist, int32_t* pred, int32_t* root_local, float* tree_dist,
                               int32_t* branch_parent, int32_t* branch_off, int32_t* branch_len, int32_t* n_branches,
                               int32_t* path_verts, int32_t* branch_of, int64_t* stats_host, void* ws, int64_t ws_bytes,
                               void* stream, const int64_t* tuning /*NULL = defaults; 24 entries, see csrc/skeleton.hip "Tuning of
                               one call": per-call strategy / sweep knobs (no process-global state)*/);
int st_post_process_seg(int n_trees, const int32_t* tree_off, const int32_t* parent, const int32_t* start, const int32_t* len,
                        float* xyz, const float* rad_in, float* rad_out, uint8_t* keep, uint8_t* repaired, uint8_t* smoothed,
                        int32_t* depth_scratch, int do_prune, float min_radius, float min_length, int do_repair,
                        int do_smooth, int kernel_size, const int32_t* first_tree /*[n_first] first tree of every cloud*/,
                        int n_first, void* stream);

/* ---- training / evaluation losses ----------------------------------------
 * replaces: compute_loss + L1Loss + cosine_similarity_loss + focal_loss + dice_loss (smart_tree/model/loss.py:7-97) as ONE
 *           pass over the voxels.  radius [n], direction [n,3], class_l [n,C] are the network's outputs; targets [n,5] =
 *           (radius, direction xyz, class id); mask [n] uint8 or NULL; vector_class < 0 = None.
 * out_host[8] (the call waits for the stream): radius, direction, focal, dice loss; vector rows; class rows; 0; 0.
 * An empty selection gives NaN (mean of an empty tensor).  A target class id outside [0, C) is an error (torch raises). */
int64_t st_loss_workspace_bytes(void);
int st_loss_forward(const float* radius, const float* direction, const float* class_l, int n_classes, const float* targets,
                    int target_cols, const uint8_t* mask, int64_t n, int vector_class, int target_radius_log,
                    double* out_host, void* ws, int64_t ws_bytes, void* stream);

/* st_loss_backward: d radius [n] (d_radius may be NULL), d direction [n,3], d class_l [n,C] of the same four terms, weighted by
 * upstream[4] (DEVICE: radius, direction, focal, dice weights -- autograd's incoming gradients, no host synchronisation).
 * n_vector_rows / n_class_rows = out_host[4] / out_host[5] of the forward.  Unselected rows get zeros.  Enqueue only. */
int st_loss_backward(const float* radius, const float* direction, const float* class_l, int n_classes, const float* targets,
                     int target_cols, const uint8_t* mask, int64_t n, int vector_class, int target_radius_log,
                     double n_vector_rows, double n_class_rows, const float* upstream, float* d_radius, float* d_direction,
                     float* d_class_l, void* stream);

/* ---- training: sparse-convolution weight gradient, float32 and half features (csrc/sparse_conv_grad.hip) ---------
 * replaces: the weight-gradient half of spconv's backward (what autograd runs through SubMConv3d / SparseConv3d /
 *           SparseInverseConv3d in smart_tree/model/train.py:24-58).  The data gradient is st_sparse_conv_fwd over the transposed
 *           table (smart_tree_amd/model/sparse_grad.py).
 * dw[k][ci][co] = sum over o < n_out with nbr[k][o] >= 0 of cat(x0, x1)[nbr[k][o]][ci] * dy[o][co]; dw is [K][cin][cout] (w's
 * layout in st_sparse_conv_fwd).  nbr NULL = pointwise (K = 1); nbr_stride 0 = n_out; n_out == 0 writes zeros.
 * Deterministic: no float atomics, partial sums per (row chunk, offset) in ws, added in chunk order.  cin + cout <= 8192.
 * st_sparse_conv_wgrad_h (declared with the half calls below) is the same scheme for half x0 / x1 / dy. */
int64_t st_sparse_conv_wgrad_workspace_bytes(int K, int cin, int cout, int64_t n_out);
int st_sparse_conv_wgrad(const float* x0, int c0, const float* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                         int64_t nbr_stride, const float* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream);

/* ---- mixed-precision (autocast float16) training (csrc/sparse_conv_half.hip; the weight gradient: csrc/sparse_conv_grad.hip) ----
 * replaces: spconv's half-precision conv forward and backward under torch.cuda.amp.autocast (model/train.py:24-58 with
 *           conf/training.yaml fp16: True): SubMConv3d / SparseConv3d / SparseInverseConv3d, model/model_blocks.py:8-285.
 * st_sparse_conv_h_fwd: y = sum_k cat(x0, x1)[nbr[k]] . W[k]; x0, x1, w [K][cin][cout] (plain layout) and y are IEEE half, the
 * sums float32, one rounding to half at the store; no epilogue.  Any cin, cout >= 1 and concat split (as st_sparse_conv_fwd's
 * generic kernel); nbr NULL = pointwise (K = 1); nbr_stride 0 = n_out.  The data gradient is this call over the transposed table.
 * st_sparse_conv_wgrad_h: st_sparse_conv_wgrad with half x0 / x1 / dy; dw float32, accumulated in float32, deterministic
 * (partial slabs per (row chunk, offset) in ws, added in chunk order).  cin + cout <= 8192.
 * Neither clamps: inf / NaN operands reach every sum they take part in.
 * st_move_rows_h: st_move_rows for rows of `row_elems` 2-byte elements (1..512, odd counts included). */
int st_sparse_conv_h_fwd(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                         int64_t nbr_stride, const void* w, int cout, void* y, void* stream);
int64_t st_sparse_conv_wgrad_h_workspace_bytes(int K, int cin, int cout, int64_t n_out);
int st_sparse_conv_wgrad_h(const void* x0, int c0, const void* x1, int cin, const int32_t* nbr, int K, int64_t n_out,
                           int64_t nbr_stride, const void* dy, int cout, float* dw, void* ws, int64_t ws_bytes, void* stream);
int st_move_rows_h(const void* src, int row_elems, const int32_t* order, int64_t n, void* dst, int scatter, void* stream);

/* ---- training: BatchNorm over [n, C] rows, synchronised across ranks (csrc/batchnorm.hip) ----------------
 * replaces: torch.nn.BatchNorm1d's training forward and backward (model_blocks.py), with the batch statistics of the whole global
 *           batch: the caller all-reduces the small float64 vectors between the passes (smart_tree_amd/model/sync_bn.py).
 * half = 0: x / dy / y / dx float32; half = 1: IEEE half, float32 math.  mean, invstd, gamma, beta are float32 [C] device vectors.
 * st_bn_stats:           out [2C + 1] float64 = sum x | sum x^2 | n.
 * st_bn_apply:           y = (x - mean) * invstd * gamma + beta.
 * st_bn_backward_stats:  out [2C] float64 = sum dy | sum dy * xhat, xhat = (x - mean) * invstd recomputed from x.
 * st_bn_backward_apply:  dx = gamma * invstd * (dy - sum_dy / N - xhat * sum_dy_xhat / N); sums [2C] and count [1] (= N) are float64
 *                        device values (the all-reduced backward stats and the forward's global row count).
 * The two stats calls are deterministic: per-chunk partials in ws (st_bn_workspace_bytes), added in a fixed order, no float
 * atomics.  n = 0 launches no kernel (the stats calls zero `out`).  1 <= C <= 4096.  Enqueue only. */
int64_t st_bn_workspace_bytes(int64_t n, int C);
int st_bn_stats(const void* x, int half, int64_t n, int C, double* out, void* ws, int64_t ws_bytes, void* stream);
int st_bn_apply(const void* x, int half, int64_t n, int C, const float* mean, const float* invstd, const float* gamma,
                const float* beta, void* y, void* stream);
int st_bn_backward_stats(const void* x, const void* dy, int half, int64_t n, int C, const float* mean, const float* invstd,
                         double* out, void* ws, int64_t ws_bytes, void* stream);
int st_bn_backward_apply(const void* x, const void* dy, int half, int64_t n, int C, const float* mean, const float* invstd,
                         const float* gamma, const double* sums, const double* count, void* dx, void* stream);

/* ---- dataset: labelled synthetic trees sampled on the device (csrc/synthetic.hip) ------------------------
 * replaces: the reference's external `synthetic-trees` download as the source of labelled trees, and the host sampler
 *           smart_tree_amd/synthetic.py:sample_tree_cloud plus the upload of its result.
 * st_synth_points_seg generates B <= 64 trees in one launch.  Device arrays, the trees' rows concatenated: table [S,16] float32
 * (ax ay az ra | bx by bz rb | ux uy uz branch-id as int32 bits | vx vy vz 0), cdf [S] uint32 (floor(2^32 * cumulative lateral
 * area / total), a tree's last entry 0xFFFFFFFF), tips [T,3] float32.  HOST arrays (they travel as kernel arguments, so the call
 * checks them and is still enqueue-only): tab_off, tip_off, pt_off [B+1] int32 (tree s owns rows [tab_off[s], tab_off[s+1]) and
 * points [pt_off[s], pt_off[s+1]), pt_off[0] = 0), seeds [B] uint64, fol_thr [B] uint32 (min(floor(fraction * 2^32), 2^32 - 1);
 * all ones = every point), noise and foliage_sigma [B] float32.  Point i of a tree draws from Philox4x32-10 with key = the two
 * halves of the seed and counter (i, k, 0, 0), k = 0, 1; the use of each word and the float32 evaluation order are the table in
 * the header comment of csrc/synthetic.hip.  Outputs (device, each nullable): xyz, medial_vector [N,3], class_l [N] float32
 * (1 = foliage), branch_ids [N] int32 (-1 foliage), segment [N] int32 (row of the batched table, -1 foliage); N = pt_off[B].
 * Refused, nothing written: B > 64, a negative or decreasing offset, a tree with points and no segments.
 * st_synth_philox (host, for tests): out[4] = Philox4x32-10(counter[4], key[2]), the function the kernel calls. */
int st_synth_points_seg(const float* table, const int32_t* tab_off, const uint32_t* cdf, const float* tips, const int32_t* tip_off,
                        const int32_t* pt_off, int B, const uint64_t* seeds, const uint32_t* fol_thr, const float* noise,
                        const float* foliage_sigma, float* xyz, float* medial_vector, float* class_l, int32_t* branch_ids,
                        int32_t* segment, void* stream);
void st_synth_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* ---- evaluation: per-point prediction metrics (csrc/prediction_metrics.hip) ------------------------------
 * replaces: nothing in the reference (no evaluation of the network's outputs exists there); reads the rows st_loss_forward
 *           reads, once: radius [n], direction [n,3], class_l [n,C] (predictions), targets [n,5] = radius, direction xyz, class id,
 *           mask [n] bytes or NULL.  Segment s (a tree of the batch) owns rows [seg_off_host[s], seg_off_host[s+1]); NULL with
 *           n_seg = 1 is the one segment [0, n).  seg_off_host, thr_host [n_thr] and edges_host [n_edges] are HOST arrays (they
 *           travel as kernel arguments: the call checks them and is still enqueue-only; nothing is read back).
 * Per selected row (mask NULL or non-zero), float32 in the order written in the header of csrc/prediction_metrics.hip:
 *   target class tc = (int)t[4], valid iff t[4] > -1 && t[4] < C (else bad_class, nothing more); predicted class pc = the first
 *   NaN logit if any, otherwise the first largest; confusion[tc][pc] (target row, prediction column).  For vector rows
 *   (vector_class < 0 or tc == vector_class): r_gt = t[0], r_pred = target_radius_log ? expf(radius) : radius, dr = |r_pred - r_gt|,
 *   ang = acosf(clamp(p^ . q^, -1, 1)) with norms clamped at 1e-8f, err = |r_pred p^ - r_gt q^| (the distance between the
 *   predicted and the labelled medial point); a row with a non-finite dr, dr / r_gt, ang, err or err / r_gt counts in
 *   bad_vector only; otherwise within[j] counts err <= thr[j] * r_gt and the row falls into radius bin #{e: r_gt >= edges[e]}.
 * Record of a segment, n_bins = n_edges + 1 (both tallies are DEVICE arrays of n_seg records, fully written by the call):
 *   tally_ints  int64   confusion[C*C] | bad_class | vector_rows | bad_vector | rows | within[n_thr] | bin_count[n_bins]
 *   tally_sums  double  sum dr | sum dr/r_gt | sum ang | sum err | sum err/r_gt | bin_dr_rel[n_bins] | bin_err_rel[n_bins]
 *   (rows = selected rows; vector_rows = the rows in the sums).  st_prediction_metrics_tally_ints / _tally_sums give the entries
 *   of one record (-1 beyond the limits).  Integer atomics and float64 partials added in a fixed order: a segment's record is bit
 *   for bit the record of the same rows evaluated alone, and two calls give the same bits.  n == 0 or an empty segment: zeros.
 * Limits: 1 <= C <= 16, n_thr <= 16, n_bins <= 16, 1 <= n_seg <= st_abi_entries(2).  Refused, nothing launched or written: a limit
 *   exceeded, target_cols != 5, edges not finite or not strictly ascending, a NaN threshold, offsets that decrease, do not start
 *   at 0 or do not end at n, a null input with n > 0, a workspace below st_prediction_metrics_workspace_bytes(n, n_seg, n_bins). */
int64_t st_prediction_metrics_tally_ints(int n_classes, int n_thr, int n_bins);
int64_t st_prediction_metrics_tally_sums(int n_bins);
int64_t st_prediction_metrics_workspace_bytes(int64_t n, int n_seg, int n_bins);
int st_prediction_metrics(const float* radius, const float* direction, const float* class_l, int n_classes,
                          const float* targets, int target_cols, const uint8_t* mask, int64_t n,
                          const int64_t* seg_off_host, int n_seg, int vector_class, int target_radius_log,
                          const float* thr_host, int n_thr, const float* edges_host, int n_edges,
                          int64_t* tally_ints, double* tally_sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- rendering: clouds and skeletons to images (csrc/render.hip) -------------------------------------------
 * replaces: o3d_abstractions/camera.py:71-101 (Renderer.capture: open3d's OffscreenRenderer) and the to_o3d_* geometry built for
 *           it (model/render.py:7-35).  A frame is: st_render_clear, any number of st_render_points / st_render_segments calls (each
 *           with its own id range, in the order of the frame's items), st_render_resolve.  All of them take the SAME workspace of
 *           st_render_workspace_bytes(V, H, W) bytes: it holds the framebuffer [V,H,W] of 64-bit keys = (bits of the positive
 *           float32 depth) << 32 | id, min-reduced with one atomic per covered pixel -- the nearest surface wins, equal depths go
 *           to the lowest id, and the result does not depend on the order of arrival (bit-identical from call to call).
 * cams [V,16] float32 DEVICE: R (9, row-major), t (3), fx, fy, cx, cy.  Camera space is R p + t, +z forward; pixel (column u, row v)
 *   has its centre at the integer (u, v).  The float32 operation order is the header comment of csrc/render.hip.
 * st_render_points: xyz [n,3], radius [n] world radii or NULL.  A point goes to its nearest pixel and covers the disc of
 *   max(point_px/2, fx r / z) pixels around its projection (point_px = 1: exactly one pixel); depth z.  Culled: z <= near,
 *   non-finite coordinates, off the viewport.  Ids id_base + i.
 * st_render_segments: a, b [m,3], r1, r2 [m]: screen-space capsules between the projected ends (clipped at z = near, radius
 *   interpolated) with pixel radii max(fx r / z, min_px/2), depth of a sphere impostor around the perspective-correct axis point,
 *   never below near.  Skeleton tubes, and with radius 0 and min_px = 1 lines one pixel wide.  Ids id_base + i.
 * st_render_resolve: rgb uint8 [V,H,W,3], depth float32 [V,H,W] (+inf on the background), ids int32 [V,H,W] (-1); each may be NULL.
 *   items_host [n_items] (HOST; it travels as a kernel argument) says who owns the ids, in order, and how they are coloured -- the
 *   colour is looked up per visible pixel.  An id no item owns is black.  edl_strength > 0: eye-dome shading from the depths of the
 *   4 neighbours at edl_px.  Background is white.
 * Refused, nothing launched: V < 1 or > 65536, W or H < 1 or > 16384, a null input with a count above 0, null cameras, ids that
 *   reach 2^31, near / point_px / min_px / edl_strength negative or not finite (near must be > 0), more than 16 items, a class
 *   item without a colour map, a workspace below st_render_workspace_bytes (-1 for a refused view).  No write happens outside the
 *   three images and the workspace, whatever the coordinates. */
#define ST_RENDER_UNIFORM 0 /* rgb */
#define ST_RENDER_RGB 1     /* data: float32 [count,3] */
#define ST_RENDER_CLASS 2   /* data: int32 [count], cmap: float32 [n_classes,3]; a class outside [0, n_classes) is black */
#define ST_RENDER_SCALAR 3  /* data: float32 [count] through the blue-cyan-green-yellow-red ramp over [lo, hi] */
#define ST_RENDER_ID 4      /* data: int32 [count] through a hash (branch ids) */
typedef struct StRenderItem {
    int64_t count; /* ids owned by the item: points or segments drawn for it */
    int32_t mode, n_classes;
    const void* data;  /* DEVICE */
    const float* cmap; /* DEVICE */
    float lo, hi;
    float rgb[3];
    float reserved;
} StRenderItem;
int64_t st_render_workspace_bytes(int V, int H, int W);
int st_render_clear(int V, int H, int W, void* ws, int64_t ws_bytes, void* stream);
int st_render_points(const float* xyz, const float* radius, int64_t n, int64_t id_base, float point_px, const float* cams, int V,
                     int H, int W, float near, void* ws, int64_t ws_bytes, void* stream);
int st_render_segments(const float* a, const float* b, const float* r1, const float* r2, int64_t m, int64_t id_base, float min_px,
                       const float* cams, int V, int H, int W, float near, void* ws, int64_t ws_bytes, void* stream);
int st_render_resolve(const StRenderItem* items_host, int n_items, int V, int H, int W, float edl_strength, int edl_px,
                      uint8_t* rgb, float* depth, int32_t* ids, void* ws, int64_t ws_bytes, void* stream);

/* ---- skeleton stage: bridging components across gaps (csrc/bridge.hip) -------------------------------------
 * The reference stops short of this (skeleton/connection.py is a stub, data_types/tree.py:connect only draws a line): a branch
 * whose medial points are cut by occlusion comes back as separate trees.  The bridges are edges to ADD TO THE GRAPH before the
 * shortest-path stage.
 *
 * Input: the layout of st_component_layout_seg -- vert_order [m] (original ids of the kept vertices, components contiguous),
 * new_id [n], comp_off [n_comp + 1], and for a batch vert_seg_off [nseg + 1], the clouds' ranges in the renumbered vertex space
 * (NULL / nseg = 1: one cloud) -- and the vertex positions pts [n,3].  Only kept vertices take part.
 * Candidates: vertex pairs in different components of one cloud with d2 <= max_gap * max_gap (float32 product, formed once),
 * d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction.  Strict total order (bits of d2, lo id, hi id).  The bridges are
 * the minimum spanning forest of the component graph under that order: edges [B,2] int64 (original ids, lo < hi), weights [B] =
 * sqrtf(d2), in the order of the components they hook; B <= n_comp - 1 <= cap is written to *n_bridges_host.
 * stats_host (optional, 4 x int64, zeroed and written): Boruvka rounds, boundary vertices of round 1, bridges, 0.
 * m = 0, n_comp <= 1 or max_gap <= 0 (or NaN): zero bridges, nothing launched.  Waits for the stream once per round. */
int64_t st_bridge_components_workspace_bytes(int64_t m, int64_t n_comp, int nseg);
int st_bridge_components_seg(const float* pts, int64_t n, const int32_t* vert_order, int64_t m, const int32_t* new_id,
                             const int32_t* comp_off, int64_t n_comp, const int32_t* vert_seg_off, int nseg, float max_gap,
                             int64_t* edges, float* weights, int64_t cap, int64_t* n_bridges_host, int64_t* stats_host, void* ws,
                             int64_t ws_bytes, void* stream);

/* ---- segmentation: every point to the tube of its cloud's skeleton it belongs to (csrc/segment.hip) --------------------
 * replaces: util/queries.py:139-166 (skeleton_to_points) where a caller wants to know WHICH tube, tree and branch, not only how far.
 *
 * Tubes in `to_tubes()` order: a, b [m,3] end points, r1, r2 [m] end radii.  Per pair, float32 in k_nearest_tube's operation order:
 * ab = b - a; dot = (x*x' + y*y') + z*z'; t = clip01(dot(ap, ab) / dot(ab, ab)); q = a + t*ab; r = (1 - t)*r1 + t*r2; v = q - p;
 * residual = sqrtf(dot(v, v)) - r (negative inside the tube); score = |residual|.  A zero-length tube is the point a (t = 0); a tube
 * with a non-finite end point or radius never wins, nor does a NaN score; a point with a non-finite coordinate gets no tube.
 * Winner: the minimum of (bits of score, tube index).  max_distance >= 0: a best score > max_distance leaves the point unassigned
 * (max_distance < 0: unbounded).  Unassigned: tube -1, residual +inf, vec 0, rad NaN.
 * Point i of cloud s (pt_seg_off [nseg + 1]) sees the tubes [tube_seg_off[s], tube_seg_off[s + 1]); NULL offsets with nseg = 1: one
 * cloud.  tube [n] is the position in the batched tube array.  m = 0 or a cloud without tubes: its points are unassigned.
 * Every per-point output may be NULL.  tally (optional, [3*m] int64, zeroed by the call), per tube: points won, sum of
 * llrintf(score * 2^24), sum of llrintf(residual * 2^24) (the scaled value clamped to +-2^62): integer sums, bit-identical
 * from run to run and between the forms.
 * form: 1 dense (every point against every tube of its cloud), 2 grid (the tubes binned into a per-cloud grid, a point walks the
 * shells of cells around it until a float32-safe lower bound ends the search), 0 auto (by m / nseg).  The forms give identical bits.
 * Enqueue-only.  Refused, nothing launched: n or m outside [0, 2^31), nseg outside [1, st_abi_entries(2)], nseg > 1 without both
 * offset arrays, a NaN max_distance, a form outside 0..2 (-1); a workspace below st_segment_workspace_bytes(n, m, nseg) (-2; the
 * size query returns -1 for sizes the call refuses).  After a grid call the first four int64 of the workspace hold: points that
 * walked the grid, the sum and the maximum of the shells they visited, points that ended in a plain sweep. */
int64_t st_segment_workspace_bytes(int64_t n, int64_t m, int nseg);
int st_segment_points_seg(const float* pts, int64_t n, const int32_t* pt_seg_off, const float* a, const float* b, const float* r1,
                          const float* r2, int64_t m, const int32_t* tube_seg_off, int nseg, float max_distance, int form,
                          int32_t* tube, float* residual, float* vec, float* rad, int64_t* tally, void* ws, int64_t ws_bytes,
                          void* stream);

/* ---- fitting: every tube to the points segmented onto it (csrc/fit.hip) -------------------------------------------------
 * replaces: nothing -- the reference's radii are the network's prediction, corrected by the box filter of `smooth` only.
 *
 * pts [n,3]; tube [n] int32 as st_segment_points_seg wrote it (a position in the tube arrays; -1 or any value outside [0, m):
 * the point takes no part); a, b [m,3], r1, r2 [m].  Per tube, float32, no contraction:
 *   frame: ab = b - a; k = the coordinate with the smallest |ab_k| (ties to the lowest); e1 = normalise(cross(ab, unit_k)),
 *   e2 = normalise(cross(ab, e1)), normalise(x) = x / sqrtf(dot(x, x)), dot = (x*x' + y*y') + z*z'.
 *   a point enters when it is finite, q = dot(p - a, ab) / dot(ab, ab) satisfies 0 <= q <= 1 (never for a zero-length tube; a point
 *   past an end cap is left out), rho = the distance to the axis at q is > 0, and max_relative < 0 or
 *   |rho - r(q)| <= max_relative * r(q) with r(q) = (1 - q)*r1 + q*r2.
 *   it adds, with w the unit vector from the axis to the point, c = dot(w, e1), s = dot(w, e2): moments [10*m] int64 (optional),
 *   per tube the count and the sums of llrintf(x * 2^24), the scaled value clamped to +-2^40, of c*c, c*s, s*s, c, s, rho*c, rho*s,
 *   rho, rho*rho: integer sums, bit-identical from run to run.
 * The solve (float64, from the integer moments): one Gauss-Newton step of the geometric circle fit, the least squares of
 * rho_i - (c_i, s_i).(cu, cv) - R = 0.  spread = the smaller eigenvalue of the covariance of (c, s).
 * fit [8*m] float64 (optional), per tube: N, R, the offset cu*e1 + cv*e2 (3), the rms of the linear residual, the spread, the status:
 *   0 not fitted (N < min_points; the rest of the row is 0), 1 radius only (spread < min_spread: R = the mean of rho, offset 0),
 *   2 full fit.
 * Enqueue-only.  n = 0 or m = 0 launches no kernel and zeroes the outputs.  Refused, nothing launched: n or m outside [0, 2^31),
 * a NaN max_relative or min_spread, a missing input array (-1); a workspace below st_fit_tubes_workspace_bytes(n, m) (-2; the size
 * query returns -1 for sizes the call refuses). */
int64_t st_fit_tubes_workspace_bytes(int64_t n, int64_t m);
int st_fit_tubes(const float* pts, int64_t n, const int32_t* tube, const float* a, const float* b, const float* r1, const float* r2,
                 int64_t m, float max_relative, int64_t min_points, double min_spread, int64_t* moments, double* fit, void* ws,
                 int64_t ws_bytes, void* stream);

/* ---- inventory: what every tree of a segmented cloud occupies (csrc/tree_tally.hip) --------------------------------------
 * replaces: nothing -- the reference measures no tree (BranchSkeleton.length / TreeSkeleton.length are its only quantities).
 *
 * pts [n,3]; tree [n] int32, the row of the point's tree among n_trees = T (a batch: rows of all its clouds' trees); cls [n] uint8
 * or NULL (NULL: one class, n_classes is read as 1 and every point is class 0).  Point i takes part when its three coordinates
 * are finite, 0 <= tree[i] < T and (cls == NULL or cls[i] < n_classes).
 * box [6*T] float32: per tree the minimum then the maximum of x, y, z over its points, compared through the order-preserving
 *   integer map of the float's bits (-0 orders below +0); a tree without points keeps (+inf x3, -inf x3).
 * counts [T*n_classes] int64: points per tree and class.
 * Cell of a point, in its tree's own box, float32 without contraction: i_k = (int)floorf((p_k - min_k) / cell), clamped to
 *   [0, 16383].  up in 0..2 is the vertical axis (the package's convention is 1); the point's layer is min(i_up, layers - 1).
 * area_cells [T] int64: the distinct pairs of the two horizontal indices among the tree's points.
 * profile [T*layers] int64: per layer the distinct index triples whose layer it is; triples above the last layer stay distinct
 *   and are counted in the last layer.
 * Every output may be NULL; a NULL area_cells or profile skips that family of keys.  All outputs are integers or extrema: identical
 * bits from run to run, and for a batch and its clouds taken alone (a tree's rows depend on its own points only).
 * Enqueue-only, no read-back.  n = 0 or T = 0 launches nothing beyond the fills of the outputs.  Refused, nothing launched or
 * written: n outside [0, 2^31), T outside [0, 2^21), layers outside [1, 4096], up outside 0..2, a cell that is not finite or not
 * > 0, n_classes outside [1, 255], a NULL pts or tree with n > 0 (-1); a workspace below st_tree_tally_workspace_bytes(n, T, layers)
 * (-2; the size query returns -1 for sizes the call refuses).  The workspace holds the set of distinct cells at its worst case,
 * every point in a cell of its own in both families, at most half full: 32 bytes per point rounded up to a power of two. */
int64_t st_tree_tally_workspace_bytes(int64_t n, int64_t n_trees, int layers);
int st_tree_tally(const float* pts, int64_t n, const int32_t* tree, const uint8_t* cls, int n_classes, int64_t n_trees, int up,
                  float cell, int layers, float* box, int64_t* counts, int64_t* area_cells, int64_t* profile, void* ws,
                  int64_t ws_bytes, void* stream);

/* ---- terrain: a ground raster under a cloud, ground points and height above ground (csrc/ground.hip) ----------------------
 * replaces: nothing -- the reference's clouds hold trees only and it has no notion of terrain.
 * A progressive morphological filter (Zhang et al. 2003) on a raster of per-cell minima.  Every step is a minimum, a maximum, one
 * float32 subtraction or one comparison: the outputs are identical bits from run to run, and for a batch and its clouds alone.
 *
 * Batch: seg_off [nseg + 1] int32 (device) gives the clouds of the points (NULL with nseg = 1), 1 <= nseg <= st_abi_entries(2).
 * Every cloud has a raster of its own; the rasters lie one behind the other, cloud s at cell_off[s] (int64 [nseg + 1], HOST).
 * up in 0..2 is the vertical axis; the plan axes a < b are the other two.  A point takes part when its three coordinates are
 * finite.  "Ordered" means compared through the order-preserving integer map of the float's bits (-0 below +0).
 * origin [2 * nseg] float32 (device): per cloud the ordered minimum of the a and of the b coordinate of its participating points.
 * Cell of a point: ia = (int)floorf((pa - a0) / cell), ib likewise -- one float32 subtraction, one float32 division.
 * dims [2 * nseg] int32: A = max ia + 1, B = max ib + 1 (at most 2^30); the linear index of a cell is ia * B + ib.  A cloud
 * without a participating point has origin (+inf, +inf) and dims (0, 0).
 *
 * st_ground_extent writes origin and dims (both device).  Enqueue-only; workspace st_ground_workspace_bytes(0).
 *
 * st_ground_model: origin on the device as st_ground_extent left it; dims [2 * nseg] int32 and cell_off on the HOST; K = n_windows
 * in 1..16 half-widths w [K] int32 (HOST) in cells, strictly increasing, each in 1..32; thresholds dh [K] float32 (HOST; no NaN).
 * Writes surface [cells] float32 and flags [cells] uint8: bit 0 = no point in the cell, bit 1 = not ground.
 *   1. Z[c] = the ordered minimum of the up-coordinates of the points of cell c, +inf for a cell without points (bit 0).  A point
 *      whose cell is outside dims takes no part (none is with the extent's own answer).
 *   2. For k = 0 .. K-1, with the square window of half-width w[k] clipped at the raster's edge:
 *        E[c] = the ordered minimum of Z over the window (+inf is neutral);
 *        O[c] = the ordered maximum of E over the window over finite E only, +inf when there is none;
 *        if Z[c] - O[c] > dh[k] (one float32 subtraction, a strict comparison): set bit 1 and Z[c] = O[c].
 *      All cells of a window read the Z the previous window left.  An empty cell is filled by the first window that reaches data
 *      (inf - finite > dh; a window reaches 2 w cells, w for E and w for O) and stays +inf when nothing is in reach (inf - inf is
 *      NaN, which is not greater).
 *   3. surface = Z after the last window.
 * Enqueue-only; workspace st_ground_workspace_bytes(cells) (12 bytes per cell; -1 for cells outside [0, 2^26]).
 *
 * st_ground_height: m query positions pts [m,3] with their own seg_off (the cloud itself or any other positions) against the
 * rasters.  Writes height [m] float32, is_ground [m] uint8 and ground [m] float32, each of which may be NULL.
 *   qa = (pa - a0) / cell; ia = (int)floorf(qa) clamped into [0, A - 1]; ib likewise; own = surface[ia, ib].
 *   is_ground = (p_up - own <= tol): one float32 subtraction.
 *   fa = qa - 0.5f, i0 = floorf(fa), ta = fa - i0 (single float32 operations in this order), likewise fb, j0, tb; the indices i0,
 *   i0 + 1, j0, j0 + 1 are clamped into the raster (as floats, before the conversion); a sample that is not finite is replaced
 *   by own; s0 = S[i0,j0] + tb (S[i0,j1] - S[i0,j0]), s1 = S[i1,j0] + tb (S[i1,j1] - S[i1,j0]), ground = s0 + ta (s1 - s0),
 *   height = p_up - ground, in float32 without contraction.
 *   A point that does not take part, one of a cloud without cells, or one whose own cell is +inf: height and ground NaN,
 *   is_ground 0.
 * Enqueue-only, no workspace.
 *
 * Refused by all three, nothing launched or written (-1; the text starts with "ground_extent:", "ground_model:" or
 * "ground_height:"): a cell that is not finite or not > 0, up outside 0..2, nseg outside [1, st_abi_entries(2)] or nseg > 1 without
 * seg_off, points outside [0, 2^31), NULL points with n > 0, NULL outputs (extent) or NULL surface / flags with cells > 0; by model
 * and height: NULL origin, dims or cell_off, a side outside [0, 16384] or only one side 0, more than 2^26 cells, a cell_off that
 * is not the running sum of A * B from 0; by model: K outside 1..16, windows not strictly increasing or outside 1..32, a NaN
 * threshold; by height: a NaN tol.  A workspace below the size query's answer: -2. */
int64_t st_ground_workspace_bytes(int64_t cells);
int st_ground_extent(const float* pts, int64_t n, const int32_t* seg_off, int nseg, int up, float cell, float* origin, int32_t* dims,
                     void* ws, int64_t ws_bytes, void* stream);
int st_ground_model(const float* pts, int64_t n, const int32_t* seg_off, int nseg, int up, float cell, const float* origin,
                    const int32_t* dims_host, const int64_t* cell_off_host, int n_windows, const int32_t* w_host, const float* dh_host,
                    float* surface, uint8_t* flags, void* ws, int64_t ws_bytes, void* stream);
int st_ground_height(const float* pts, int64_t m, const int32_t* seg_off, int nseg, int up, float cell, float tol, const float* origin,
                     const int32_t* dims_host, const int64_t* cell_off_host, const float* surface, float* height, uint8_t* is_ground,
                     float* ground, void* stream);

/* ---- virtual laser scanner: beams against the tubes of a skeleton, first hits as labelled points (csrc/scan.hip) -----------
 * replaces: nothing -- the reference has no scanner model; its training clouds are an external download.
 *
 * Tubes a, b [m,3], r1, r2 [m] (device), tube_seg_off [nseg + 1] int32 (device; NULL with nseg = 1), 1 <= nseg <= st_abi_entries(2);
 * tube_class [m] uint8 (0 wood, anything else leaf; NULL: all wood) and tube_branch [m] int32 (NULL: every branch id is -1).
 * scanners [n_scanners] and ray_off [n_scanners + 1] are HOST arrays, read before the call returns; a scanner's cloud may not
 * decrease along the table, and ray_off must be the running sum of n_az * n_el from 0.  Ray k of a scanner is beam
 * (i, j) = (k / n_el, k % n_el): az = az0 + i daz, el = el0 + j del (radians), direction (cos el cos az, cos el sin az, sin el).
 * Surface, solve, winner and the two forms: the head of csrc/scan.hip.  In short: the surface of a tube is the zero set of the
 * point-to-tube residual (frustum side and the two end spheres outside it; a zero-length tube is a sphere); a hit is the smallest
 * root s with min_range <= s <= max_range over the tubes of the scanner's cloud, ties to the lowest tube; a ray from inside a tube
 * returns its far wall; a tube with a non-finite value or a negative radius is never hit.  form: 0 auto, 1 dense, 2 grid -- the
 * same bits in every output.
 * Per ray (R = ray_off[n_scanners] rows; each may be NULL): dir [R,3], range [R] (+inf without a hit), tube [R] int32 (-1 without).
 * Per hit, compacted in ray order (room for R rows; each may be NULL): xyz [.,3] = the hit moved along the ray by range_noise x a
 * normal draw (Philox4x32-10, key = seed, counter = (k, 0, 0, 0)); medial_vector [.,3] = the axis point minus the un-noised hit
 * (0 for a leaf); class_l float32 (0 / 1); branch_ids int32 (-1 for a leaf); segment int32 (the tube); ray int32; n_hits int64 [1]
 * (device).
 * Enqueue-only: no allocation, no read-back, no wait.  Refused, nothing launched (-1): m outside [0, 2^31), nseg out of range or
 * nseg > 1 without tube_seg_off, n_scanners outside [0, ST_SCAN_MAX_SCANNERS], a scanner with a non-finite position, angle or
 * range_noise, with NaN or negative ranges or max_range < min_range, with a negative beam count or a cloud out of range or below
 * its predecessor's, 2^31 - 1 beams or more, a ray_off that is not the running sum, a form outside 0..2; a workspace below
 * st_scan_cast_workspace_bytes(R, m, n_scanners, nseg) (-2; the size query returns -1 for sizes the call refuses). */
#define ST_SCAN_MAX_SCANNERS 4096 /* the table travels as kernel arguments, 32 scanners per launch: 129 small launches at the limit */
typedef struct StScanner {
    int32_t cloud, n_az, n_el, reserved;
    float position[3];
    float az0, daz, el0, del;
    float min_range, max_range, range_noise;
    uint64_t seed;
} StScanner;
int64_t st_scan_cast_workspace_bytes(int64_t n_rays, int64_t m, int n_scanners, int nseg);
int st_scan_cast_seg(const float* a, const float* b, const float* r1, const float* r2, int64_t m, const int32_t* tube_seg_off, int nseg,
                     const uint8_t* tube_class, const int32_t* tube_branch, const StScanner* scanners, int n_scanners,
                     const int64_t* ray_off, int form, float* dir, float* range, int32_t* tube, float* xyz, float* medial_vector,
                     float* class_l, int32_t* branch_ids, int32_t* segment, int32_t* ray, int64_t* n_hits, void* ws, int64_t ws_bytes,
                     void* stream);

/* Beam occupancy (csrc/occupancy.hip): every beam of a scan walked through a voxel grid and tallied per cell.
 *
 * origins [n_origins,3] float32 (device); per beam (device, n_beams rows) origin_idx int32, dir [.,3] float32 (unit), range float32
 * (>= 0 a return, +inf no return).  grids [n_grids] and beam_off [n_grids + 1] are HOST arrays, read before the call returns:
 * beams beam_off[g] .. beam_off[g + 1] - 1 belong to grid g (beam_off[0] = 0, beam_off[n_grids] = n_beams, not decreasing);
 * 1 <= n_grids <= st_abi_entries(2), 1 <= dim <= 1024 per axis, cell > 0, fewer than 2^31 cells in all.  max_range >= 0 (+inf
 * allowed) ends every beam's free part; behind != 0 also counts, per cell, the returns that ended before it.
 * Per cell, the grids' cells concatenated in table order, cell (x, y, z) of a grid at (x dim_y + y) dim_z + z (device, zeroed by the
 * call): enter uint32 (free beams that entered), hit uint32 (returns that ended there), behind uint32, path uint64 (free path in
 * units of cell / 65536).  Per beam (may be NULL): hit_cell int32, the cell inside the beam's grid, or -1.  counters uint32 [2]
 * (device): [0] n_bad -- beams with a non-finite origin, direction or range, a negative range, an origin_idx outside the table or
 * |dir|^2 outside [0.998, 1.002]; they touch nothing -- and [1] n_outside, good beams that never touch their grid.
 * The walk, its tie and boundary rules and the chord's rounding: the head of csrc/occupancy.hip.  form: 0 auto, 1 aggregated (the
 * lanes of a wavefront that stand in one cell share one atomic per field), 2 plain -- the same bits in every output.
 * Enqueue-only: no allocation, no read-back, no wait.  Refused, nothing launched (-1): n_beams or n_origins outside [0, 2^31),
 * n_grids out of range, a grid with a dim outside 1..1024, a cell that is not finite and > 0 or a non-finite corner, 2^31 cells or
 * more, a beam_off that does not run from 0 to n_beams or decreases, a max_range that is NaN or negative, a form outside 0..2, a
 * NULL required array; a workspace below st_beam_tally_workspace_bytes(n_beams, n_grids) (-2; the size query returns -1 for
 * sizes the call refuses). */
typedef struct StVoxelGrid {
    float lo[3];
    float cell;
    int32_t dim[3];
    int32_t reserved;
} StVoxelGrid;
int64_t st_beam_tally_workspace_bytes(int64_t n_beams, int n_grids);
int st_beam_tally_seg(const float* origins, int64_t n_origins, const int32_t* origin_idx, const float* dir, const float* range,
                      int64_t n_beams, const StVoxelGrid* grids, int n_grids, const int64_t* beam_off, float max_range, int behind,
                      int form, uint32_t* enter, uint32_t* hit, uint32_t* behind_out, uint64_t* path, int32_t* hit_cell,
                      uint32_t* counters, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMARTTREE_HIP_H */
