/*
 * pcops.h -- C ABI of libpcops.so: the MI355X (gfx950) point-cloud operator library.
 *
 * Drop-in boundary for the native layer of the reference's PointNet++ tf_ops and
 * the DGCNN kNN-graph path.  Every entry point keeps the scalar/pointer list and
 * argument meaning of the launcher it replaces (cited per function; paths are
 * relative to the reference's pointnet2/tf_ops/), adds an explicit stream, and
 * returns a status instead of void.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP), fp32 / int32, dense row-major, the
 *     (B,N,3) AoS layout of the reference at the boundary;
 *   - the caller owns every buffer; the library never allocates, frees or
 *     synchronises; work is enqueued on `stream` (a hipStream_t passed as void*,
 *     NULL = the null stream);
 *   - gradient launchers zero their output themselves (the reference's glue does a
 *     cudaMemset first: grouping/tf_grouping.cpp:204, sampling/tf_sampling.cpp:174,
 *     3d_interpolation/tf_interpolate.cpp:258);
 *   - return PCOPS_OK (0) or a negative pcops_status; argument checks mirror the
 *     OP_REQUIRES of the reference's OpKernels;
 *   - re-entrant.  The only process-wide mutable state is the pair of switches below (pcops_set_deterministic,
 *     pcops_set_option): both are atomics read at the START of every call, so a caller that wants a per-call choice
 *     sets the option, issues the call and may restore it; kernels already enqueued are not affected.
 */
#ifndef PCOPS_H
#define PCOPS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void *pcops_stream_t; /* hipStream_t */

/* A COMPACTED row set for the grouped shared MLP (see "compacted rows" below): device pointers only, the struct
 * itself lives on the host and is read at call time. */
typedef struct pcops_rows {
    const void *blocks;     /* device, 16 bytes per 16-row block: int group, int row_in_group of the block's first row,
                               float weight of that row (1 unless it is row 0 of its group), int 0; 16-byte aligned */
    const int *block_start; /* device [groups + 1]: first block of every group, last entry = number of blocks */
    const int *rows;        /* device [1]: number of rows = 16 * number of blocks */
} pcops_rows_t;

typedef enum pcops_status {
    PCOPS_OK = 0,
    PCOPS_ERR_NULL_POINTER = -1,
    PCOPS_ERR_BAD_SHAPE = -2,     /* negative/zero extents where the reference rejects them */
    PCOPS_ERR_BAD_ARGUMENT = -3,  /* radius <= 0, nsample <= 0, k <= 0, k > n ... */
    PCOPS_ERR_UNSUPPORTED = -4,   /* shape outside what the gfx950 kernels are built for */
    PCOPS_ERR_LAUNCH = -5         /* hipGetLastError() != hipSuccess after the launch */
} pcops_status;

const char *pcops_strerror(int status);
int pcops_abi_version(void);

/* Arithmetic options.  Each selects between two formulations of the SAME fp32-in / fp32-out product whose results are both
 * within the parity bars of tests/ (the split forms carry all 24 mantissa bits of each operand in three bf16 pieces and
 * drop products <= 2^-24 relative; the fp16 pre-filter only rejects candidates, survivors get exact distances).  Values:
 *   PCOPS_OPT_GEMM_SPLIT_BF16          0 fp32 MFMA, 1 (default) split operands on the bf16 matrix pipe, 2 split only where
 *                                      the weight pieces stay LDS-resident       (pcops_mlp_gemm_fwd* and the dX products)
 *   PCOPS_OPT_WGRAD_SPLIT_BF16         0 / 1 (default): pcops_mlp_wgrad* of layers wider than 64 on both sides
 *   PCOPS_OPT_BWD_FUSED_DX_SPLIT_BF16  0 fp32 MFMA, 1: the dX half of pcops_mlp_bwd_fused* on the bf16 pipe, 2 (default): the dW
 *                                      half too where that is faster (layers of 65..128 columns whose input rows are read)
 *   PCOPS_OPT_KNN_F16_PREFILTER        0 / 1 (default): pcops_knn_graph* at c == 64, k <= 20, n >= 256 (seeded or not)
 *   PCOPS_OPT_DGRAD_SPLIT_BF16         0 fp32 MFMA, 1 (default): pcops_mlp_gemm_dgrad* with 128..256 dY columns on the bf16 pipe in
 *                                      64-column passes (weight pieces LDS-resident), 2: 128-column passes where they fit.  The same option
 *                                      carries pcops_mlp_gemm_dgrad_top (Kp = 128 .. 1024, Kp % 32 == 0; weights resident or streamed)
 *   PCOPS_OPT_BWD_FUSED_GRAM_WGRAD     0 (default) / 1: pcops_mlp_bwd_fused_gw* take shapes (pcops_mlp_bwd_fused_gw_groups > 0);
 *                                      measured -4 % .. +1 % time against the direct form (its vector arg-row term costs what
 *                                      the halved matrix work saves); superseded by value 2 of the option above
 *   PCOPS_OPT_SCATTER_QFORM            0 / 1 (default): the chunked feature-gradient walk of pcops_sa_scatter_bwd(_rows) takes its
 *                                      Q form -- Y is a function of fwd_Q, fwd_Wxyz, fwd_bias and the offsets, so its rows are
 *                                      not read (see there); 0 keeps the walk that reads Y
 *   PCOPS_OPT_XYZ_STATS_MOMENTS        0 (default) / 1: pcops_sa_gather_fwd(_rows) of a layer that is arithmetic in the offsets
 *                                      (no Q, no Ctr, Y == NULL, moments and stats_partial wanted) takes its statistics from
 *                                      the nine offset moments instead of summing the b m s x c outputs it never stores
 *                                      (opt-in: the statistics agree with float64 to 3e-7, but not bit for bit with the summed form)
 *   PCOPS_OPT_GRAM_SPLIT_BF16          0 fp32 MFMA / 1 (default): pcops_mlp_gram_rows over compacted rows at Kp == 128 on the bf16
 *                                      matrix pipe with split operands (six products per block, the column sums stay the fp32
 *                                      sums of the other form, bit for bit); Kp == 64 and rows == NULL keep the fp32 kernel
 *   PCOPS_OPT_POOL_TOP_ROWS_PIPELINED  0 / 1 (default): pcops_mlp_pool_top_wsparse_rows over compacted rows software-pipelined (the
 *                                      next group's rows and coefficients in flight under this group's sums, double-buffered LDS
 *                                      image, 16-byte LDS reads); same sums in the same order.  pcops_mlp_pool_top_addend_rows
 *                                      takes its wave-per-group kernel (a row's hits as ballots, the next row's W^T reads in
 *                                      flight) at every supported shape -- Kp = 64 / 128, S <= 64 and S <= 128; same rows, same
 *                                      rowmap, the former kernel's bits (DESIGN.md sections 4.21, 4.23).  0: the former kernels
 *   PCOPS_OPT_XCONV_CHANNEL_GROUPS     0 / 1 (default): pcops_xconv_fwd and pcops_xconv_dgrad_ws of more than 256 channels (more than
 *                                      16 channel tiles) spread the tiles over pcops_xconv_channel_groups workgroups per 16
 *                                      points, at most 8 tiles each; out, dlifted and dfts_grouped keep the one-group kernel's
 *                                      bits, dX is the groups' partial sums added in ascending order.
 *                                      0: one group everywhere.  Seeded by PCOPS_XCONV_GROUPS
 * pcops_set_option returns the PREVIOUS value (>= 0) or PCOPS_ERR_BAD_ARGUMENT.  The environment variables of rounds 3-4
 * (PCOPS_GEMM_BF3, PCOPS_WGRAD_BF3, PCOPS_BWD_FUSED_DX3, PCOPS_KNN_F16; round 6: PCOPS_DGRAD_BF3, PCOPS_BWD_FUSED_GW; later: PCOPS_GRAM_BF3, PCOPS_POOL_TOP_ROWS_PIPE, PCOPS_XCONV_GROUPS) only seed the initial values (test overrides). */
typedef enum pcops_option {
    PCOPS_OPT_GEMM_SPLIT_BF16 = 1,
    PCOPS_OPT_WGRAD_SPLIT_BF16 = 2,
    PCOPS_OPT_BWD_FUSED_DX_SPLIT_BF16 = 3,
    PCOPS_OPT_KNN_F16_PREFILTER = 4,
    PCOPS_OPT_DGRAD_SPLIT_BF16 = 5,
    PCOPS_OPT_BWD_FUSED_GRAM_WGRAD = 6,
    PCOPS_OPT_SCATTER_QFORM = 7,
    PCOPS_OPT_XYZ_STATS_MOMENTS = 8,
    PCOPS_OPT_GRAM_SPLIT_BF16 = 9,
    PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 10,
    PCOPS_OPT_XCONV_CHANNEL_GROUPS = 11,
    PCOPS_OPT_COUNT = 12
} pcops_option;
int pcops_set_option(int option, int value);
int pcops_get_option(int option);
/* diagnostics: the matrix pipe the calling thread's LAST matrix-product launch took (0 fp32 pipe or not a product, 1 bf16
 * pipe with split operands, 2 the one-pass backward's fp32 dW + split dX) -- what a roofline label should be priced on */
int pcops_last_launch_pipe(void);
/* ... and the variant it took, as up to n ints into out; returns the number of fields (5) or PCOPS_ERR_NULL_POINTER:
 *   [0] path   0 none yet, 1 tiled fp32 kernel, 2 wave-stream kernel, 3 one-pass backward (pcops_mlp_bwd_fused*),
 *              4 / 5 / 6 / 7 weight gradient: split-operand / producer-consumer / wave-stream / legacy split-K kernel,
 *              8 / 9 pcops_sa_scatter_bwd(_rows) over the inverse index: chunked walk with atomics ([1] = 1: its Q form,
 *              [2] sorted rows per chunk, [4] = 4 compacted rows) / owner walk (deterministic mode);  [3] of both: the slice
 *              width (64 / 32 / 16 / 8 channels) of the LDS streaming pass that ran first for the per-group outputs or the
 *              pooled form (sa_scatter_lds_kernel), 0 when none ran
 *              10..13 the EdgeConv family (csrc/edgeconv.hip and its launchers); their fields are their own:
 *              10 pcops_edge_pool_fwd(_ld):  [1] kernel: 0 generic, 1 64-group chunks over L2 (ec_fwd_kernel<0>), 2 LDS-resident
 *                 slice (ec_fwd_lds_kernel);  [2] rows of stats_partial written (0 without statistics);  [3] 1 for the instance
 *                 of kernels 1 / 2 that sums groups of more than 20 neighbours in blocks of 16;  [4] 1 for the _ld form
 *              11 pcops_edge_pool_bwd(_ld):  [1] 0 global atomics, 1 generic owner pair, 2 ordered owner pair (deterministic
 *                 mode), 3 arg-row kernel + inverse index + owner walk of edgeconv.hip, 4 the one-walk kernel
 *                 (PCOPS_EDGECONV_BWD_FUSED=1);  [2] the walk: 0 none of edgeconv.hip's, 1 lists read from global memory
 *                 (ec_walk_kernel), 2 LDS-resident (ec_walk_lds_kernel);  [3] 1 when the inverse index was assembled in LDS as
 *                 16-bit codes (ec_csr_build_kernel<true>);  [4] 1 for the _ld form
 *              12 the Q + Ctr form of pcops_sa_gather_fwd with a stored Y (ec_fwd_kernel<1>): [2] rows of stats_partial,
 *                 [4] 1 for pcops_sa_gather_fwd_ld
 *              13 the Q + Ctr form of pcops_sa_scatter_bwd (ec_tnet_ctr_kernel + ec_walk_kernel<true>): [2], [3] as for 11,
 *                 [4] 1 for pcops_sa_scatter_bwd_ld
 *              14..16 the rest of the set-abstraction launchers (csrc/gather.hip); their fields are their own:
 *              14 pcops_sa_scatter_bwd(_rows) on the LDS-accumulating kernel alone (sa_scatter_lds_kernel):  [1] slice width in
 *                 channels (64 / 32 / 16 / 8);  [2] 1 pooled single-layer form;  [3] 1 when Y is rebuilt from the forward's
 *                 Wxyz / bias rather than read;  [4] workgroups a cloud's groups are dealt to (gsplit; 1 with a feature gradient)
 *              15 pcops_sa_scatter_bwd(_rows) on the global-atomics fallback (sa_scatter_bwd_kernel):  [2] 1 pooled
 *              16 pcops_sa_gather_fwd(_rows) on the generic kernel (sa_gather_fwd_kernel):  [1] groups per workgroup (1 or 8);
 *                 [2] rows of stats_partial written (0 without statistics);  [3] 1 for the statistics-from-moments route
 *                 (sa_gather_offsets_kernel + xyz_stats_from_moments_kernel);  [4] 4 compacted rows
 *              17 pcops_mlp_bwd_fused_xyz_rows on the all-wave tile kernel (csrc/xyz_bwd_tiles.hip): [1] = 2, [2] = 64
 *              18 pcops_mlp_bwd_tiles_rows (csrc/bwd_tiles128.hip): [1] = 2, [2] = 128, [4] = 4 over compacted rows
 *   [1] split  1 when the operands are split into bf16 pieces (the one-pass backward: 1 its dX half, 2 both halves)
 *   [2] bn     output columns per block (64, 96, 128; the weight gradients: columns of their dW tile; 0 tiled)
 *   [3] wst    1 when the weights are streamed rather than resident in LDS
 *   [4] pool   pooled operand form: 0 none, 1 whole 32-row tiles, 2 arbitrary groups, 3 s4 groups (pcops_mlp_gemm_fwd_pool
 *              with S % 32 != 0), 4 compacted rows; the Gram form of the one-pass backward adds 8
 * A diagnostic like the one above: no product path reads it. */
int pcops_last_launch_plan(int *out, int n);
/* ... and 1 when it was the pooled forward that stores no Y and sums its statistics on the accumulator registers (pcops_mlp_gemm_fwd_pool
 * / _rows with Y == NULL on the split-operand, resident-weights 128-column tile), else 0.  Same plan tuple, same
 * bits as the transposing kernel, which PCOPS_POOL_FWD_ACC_STATS=0 in the environment (read once) keeps.  A diagnostic as well. */
int pcops_last_launch_acc_stats(void);

/* ------------------------------------------------------------------ sampling */
/* farthestpointsamplingLauncher(b,n,m,inp,temp,out)   sampling/tf_sampling.cpp:94,
 * kernel sampling/tf_sampling_g.cu:105-170.  inp (b,n,3) -> out (b,m) int32.
 * `temp` is the reference's (32,n) scratch.  Up to n = 16384 this implementation keeps the
 * cloud AND the running min-distances in registers and ignores it (may be NULL);
 * larger clouds take the streamed form (the reference's path beyond its LDS-resident
 * points, tf_sampling_g.cu:133-141) and need pcops_farthest_point_sample_workspace_bytes(b, n)
 * = 4*b*n bytes there (0 for n <= 16384). */
int pcops_farthest_point_sample(int b, int n, int m, const float *inp, float *temp,
                                int *out, pcops_stream_t stream);
unsigned long long pcops_farthest_point_sample_workspace_bytes(int b, int n);

/* probsampleLauncher(b,n,m,inp_p,inp_r,temp,out)   sampling/tf_sampling.cpp:65, kernels sampling/tf_sampling_g.cu:7-103,
 * launcher :197-200.  inp_p (b,n) non-negative weights, inp_r (b,m) numbers in [0,1] -> out (b,m) int32: the smallest
 * index whose cumulative weight is >= inp_r * total.  `temp` is the reference's (b,n) scratch (tf_sampling.cpp:86) and
 * receives the row cumsum; its fp32 association is the reference's (groups of four, up-/down-sweep over the group
 * totals, compensated carry across 8192-element chunks), so `out` is bit-identical, boundary cases included. */
int pcops_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp,
                      int *out, pcops_stream_t stream);

/* gatherpointLauncher(b,n,m,inp,idx,out)   sampling/tf_sampling.cpp:125, :172-181 */
int pcops_gather_point(int b, int n, int m, const float *inp, const int *idx,
                       float *out, pcops_stream_t stream);
/* scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)   sampling/tf_sampling.cpp:150, :183-192 */
int pcops_gather_point_grad(int b, int n, int m, const float *out_g, const int *idx,
                            float *inp_g, pcops_stream_t stream);

/* ------------------------------------------------------------------ grouping */
/* queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)
 * grouping/tf_grouping.cpp:66, kernel grouping/tf_grouping_g.cu:3-36.
 * xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> idx (b,m,nsample), pts_cnt (b,m).
 * Rows with no hit are written as 0 (unspecified in the reference). */
int pcops_query_ball_point(int b, int n, int m, float radius, int nsample,
                           const float *xyz1, const float *xyz2, int *idx,
                           int *pts_cnt, pcops_stream_t stream);

/* MSG form: `nscale` radii over the same (xyz1, xyz2) pair in ONE pass over the
 * dataset (pointnet_sa_module_msg issues them back to back, utils/pointnet_util.py:
 * 175-179).  radius[s], nsample[s] are HOST arrays; idx[s] / pts_cnt[s] are host
 * arrays of device pointers.  nscale <= 4. */
int pcops_query_ball_point_multi(int b, int n, int m, int nscale, const float *radius,
                                 const int *nsample, const float *xyz1,
                                 const float *xyz2, int *const *idx,
                                 int *const *pts_cnt, pcops_stream_t stream);

/* groupPointLauncher(b,n,c,m,nsample,points,idx,out)   grouping/tf_grouping.cpp:142, :40-57 */
int pcops_group_point(int b, int n, int c, int m, int nsample, const float *points,
                      const int *idx, float *out, pcops_stream_t stream);
/* groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points)  tf_grouping.cpp:173, :61-78 */
int pcops_group_point_grad(int b, int n, int c, int m, int nsample,
                           const float *grad_out, const int *idx, float *grad_points,
                           pcops_stream_t stream);

/* selectionSortLauncher(b,n,m,k,dist,outi,out)   grouping/tf_grouping.cpp:108, :83-123.
 * Full (b,m,n) outputs like the op; first k columns sorted, literal unstable order. */
int pcops_selection_sort(int b, int n, int m, int k, const float *dist, int *outi,
                         float *out, pcops_stream_t stream);
/* knn_point(k, xyz1, xyz2) of the Python wrapper (grouping/tf_grouping.py:49-74: tile + subtract + square + reduce_sum,
 * SelectionSort, slice): xyz1 (b,n,c) dataset, xyz2 (b,m,c) queries -> val (b,m,k) squared distances, idx (b,m,k).
 * dist[t] = sum_l (xyz1[t,l] - xyz2[j,l])^2 with l ascending and no contraction, then the literal selection sort above;
 * fused: a wave per query with its distance row in LDS, so neither the (b,m,n,c) difference tensor nor the (b,m,n)
 * matrix exists.  n <= 8192 (pcops_knn_point_supported); larger clouds: pcops_knn_point_dist + pcops_selection_sort. */
int pcops_knn_point_supported(int n);
int pcops_knn_point(int b, int n, int c, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx,
                    pcops_stream_t stream);
int pcops_knn_point_dist(int b, int n, int c, int m, const float *xyz1, const float *xyz2, float *dist,
                         pcops_stream_t stream);

/* ------------------------------------------------------------ 3d_interpolation */
/* threenn_cpu(b,n,m,xyz1,xyz2,dist,idx)   3d_interpolation/tf_interpolate.cpp:60-103
 * (CPU-only in the reference).  xyz1 (b,n,3) unknown, xyz2 (b,m,3) known. */
int pcops_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2,
                   float *dist, int *idx, pcops_stream_t stream);
/* threeinterpolate_cpu(b,m,c,n,points,idx,weight,out)   tf_interpolate.cpp:107-127 */
int pcops_three_interpolate(int b, int m, int c, int n, const float *points,
                            const int *idx, const float *weight, float *out,
                            pcops_stream_t stream);
/* threeinterpolate_grad_cpu(b,n,c,m,grad_out,idx,weight,grad_points)  tf_interpolate.cpp:131-153 */
int pcops_three_interpolate_grad(int b, int n, int c, int m, const float *grad_out,
                                 const int *idx, const float *weight,
                                 float *grad_points, pcops_stream_t stream);

/* ------------------------------------------------------ deterministic backward passes
 * SURVEY section 5 / reference hazard: groupPointGrad, scatteraddpoint and threeinterpolate_grad add with float
 * atomics (tf_grouping_g.cu:61-78, tf_sampling_g.cu:183-192), so two runs of the reference differ in the last bits.
 * pcops_set_deterministic(1) (or PCOPS_DETERMINISTIC=1 in the environment) makes every backward pass of this library
 * bit-reproducible: scatter-adds are taken by ONE owner per destination point that walks the point's list of source
 * rows in ascending row order.  Entry points that only exist in an atomic form (the four *_grad launchers above and
 * below, the pooled / dCtr forms of pcops_sa_scatter_bwd) then return PCOPS_ERR_UNSUPPORTED instead of silently adding
 * in arrival order; pcops_scatter_rows_sorted is their ordered replacement. */
void pcops_set_deterministic(int on);
int pcops_get_deterministic(void);

/* out[b][d][0..c) (+)= sum over the rows e of cloud b with idx[b][e] == d, in ASCENDING e, of
 *                        w[b][e] * src[b][e / div][0..c)         (w == NULL: weight 1; accumulate != 0: "+=")
 * idx (b, rows) values in [0, ndst), src (b, rows / div, ld_src), out (b, ndst, c).  One call covers
 *   groupPointGrad      rows = m*nsample, ndst = n, div = 1          (tf_grouping.cpp:173)
 *   scatteraddpoint     rows = m, ndst = n, c = 3, div = 1           (tf_sampling.cpp:150)
 *   threeinterpolate_grad  rows = 3 n, ndst = m, div = 3, w = weight (tf_interpolate.cpp:131-153)
 *   the neighbour term of pcops_edge_feature_grad  rows = n*k, ndst = n, src = grad_out + c, ld_src = 2 c
 * workspace: pcops_scatter_rows_workspace_bytes(b, rows, ndst) bytes, 8-byte aligned.
 * Limits: ndst <= pcops_scatter_rows_sorted_max_ndst() (19 968: the per-cloud counting sort lives in LDS) and
 * rows < 2^30; pcops_scatter_rows_sorted_supported(rows, ndst) is the launcher's own predicate (PCOPS_ERR_UNSUPPORTED
 * otherwise) -- callers that may fall back to the atomic form ask it first. */
unsigned long long pcops_scatter_rows_workspace_bytes(int b, int rows, int ndst);
int pcops_scatter_rows_sorted_max_ndst(void);
int pcops_scatter_rows_sorted_supported(int rows, int ndst);
int pcops_scatter_rows_sorted(int b, int rows, int ndst, int c, int div, int ld_src, const int *idx, const float *w,
                              const float *src, float *out, int accumulate, void *workspace, pcops_stream_t stream);

/* ------------------------------------------------------------- DGCNN kNN graph */
/* The reference has no native code here (dgcnn/utils/tf_util.py:638-706 is
 * matmul + top_k + gather in TF-Python); these are the native units a TF-style
 * glue would bind for the same three functions.
 * pairwise_distance: x (b,n,c) -> adj (b,n,n), D_ij = (s_i + (-2 <x_i,x_j>)) + s_j. */
int pcops_pairwise_distance(int b, int n, int c, const float *x, float *adj,
                            pcops_stream_t stream);
/* knn = top_k(-adj,k): adj (rows,n) -> nn_idx (rows,k), ascending distance, ties ->
 * lower index. */
int pcops_knn_topk(int rows, int n, int k, const float *adj, int *nn_idx,
                   pcops_stream_t stream);
/* fused pairwise_distance + knn, never materialising (n,n): x (b,n,c) -> (b,n,k) */
int pcops_knn_graph(int b, int n, int c, int k, const float *x, int *nn_idx,
                    pcops_stream_t stream);
/* the same graph, with a hint: seed (b,n,k) names k DISTINCT points per query (DGCNN: the previous layer's neighbours,
 * dgcnn/models/dgcnn.py:31-71 rebuilds the graph on every layer's features).  The largest distance to them bounds the
 * k-th nearest distance from above, so the scan rejects everything beyond it with one compare and queues a fraction of
 * the candidates; the selection and its tie rule are untouched -- nn_idx is bit for bit pcops_knn_graph's.  The
 * precondition is CHECKED per query: a seed row with an entry outside [0, n) or with a repeated entry names fewer than k
 * distinct points and is ignored (that query is scanned without a bound) -- nn_idx is pcops_knn_graph's for ANY seed.
 * seed == NULL: pcops_knn_graph.
 * (c == 64, k <= 20, n >= 256, 16-byte aligned x, seeded or not: the pairs are first evaluated in fp16 on the 16-bit
 * matrix pipe and only those whose fp16 distance minus a rigorous error bound can still enter a list get the exact fp32
 * distance -- same indices, csrc/knn.hip knn_f16_kernel; PCOPS_OPT_KNN_F16_PREFILTER = 0 keeps the fp32-MFMA kernel.)
 * pcops_knn_graph_path says which kernel a call takes and whether that kernel USES a seed: bit 0-3 the kernel
 * (1 lane-per-query VALU, 2 fp32-MFMA distances, 3 fp16 pre-filter + exact survivors), bit 4 set when a seed is honoured
 * (the VALU kernel ignores it) -- callers decide from this whether passing the previous graph pays, instead of mirroring
 * the launcher's conditions. */
int pcops_knn_graph_seeded(int b, int n, int c, int k, const float *x, const int *seed, int *nn_idx,
                           pcops_stream_t stream);
int pcops_knn_graph_path(int b, int n, int c, int k, const float *x);
/* get_edge_feature: x (b,n,c), nn_idx (b,n,k) -> out (b,n,k,2c) = [x_i | x_j - x_i] */
int pcops_edge_feature(int b, int n, int c, int k, const float *x, const int *nn_idx,
                       float *out, pcops_stream_t stream);
/* gradient of the above w.r.t. x: grad_out (b,n,k,2c) -> grad_x (b,n,c) */
int pcops_edge_feature_grad(int b, int n, int c, int k, const float *grad_out,
                            const int *nn_idx, float *grad_x, pcops_stream_t stream);
/* the x_i half of the above only: grad_x[b,i,:] = sum_s (ga - gb)[b,i,s,:] with plain stores (deterministic mode: the
 * neighbour half is pcops_scatter_rows_sorted with accumulate = 1) */
int pcops_edge_feature_grad_central(int b, int n, int c, int k, const float *grad_out, float *grad_x,
                                    pcops_stream_t stream);

/* ------------------------------------------------- shared per-point MLP (1x1 conv + BN + ReLU [+ max-pool])
 * The reference has no native code for this stage: it is a chain of TensorFlow ops per layer
 * (pointnet2/utils/pointnet_util.py:117-127 conv2d stack + reduce_max, :223-227 FP stack;
 * pointnet2/utils/tf_util.py:120-185 conv2d = tf.nn.conv2d + bias_add + batch_norm + relu, :512-531;
 * dgcnn/models/dgcnn.py:39-48).  These are the native units a TF-style glue would bind instead: one fused
 * fp32-MFMA pass per layer and direction.  All matrices row-major; X/Y rows = (batch, point, sample)
 * flattened; per-channel vectors must be 16-byte aligned and padded to a multiple of 4 floats.
 *
 * forward:   Y[M,N] = f(X)[M,K] W[K,N] + bias,  f = identity (pro_scale == NULL) or relu(x*pro_scale[k] +
 *            pro_shift[k]) (= BN+ReLU of the previous layer applied on the fly).  stats_partial (may be NULL):
 *            float [pcops_mlp_stats_rows(M)][2][N] per-row-group column sums of (Y - pivot) and (Y - pivot)^2,
 *            pivot = stat_pivot [N] (NULL: 0).  SHIFTED MOMENTS: the variance of a batch-norm layer
 *            (pointnet2/utils/tf_util.py:512-531; TensorFlow computes it in two passes) is finalised from one-pass
 *            sums, and  E[y^2] - mean^2  on fp32 partial sums loses |mean|^2 / var digits.  Any per-channel estimate of
 *            the mean within a few standard deviations -- the layer's moving mean is the natural one -- removes that:
 *            the shift is algebraically neutral (pcops_mlp_bn_finalize adds it back to the mean), every producer of
 *            forward statistics (this family, pcops_sa_gather_fwd, pcops_edge_pool_fwd) takes the same argument.
 *            ARITHMETIC of the product (rows >= 8192, K a multiple of 8): fp32 in, fp32 out, evaluated on the bf16 matrix
 *            pipe with both operands split into three bf16 pieces (x = h + m + l to 2^-25 |x|; six exact partial
 *            products, the h.h products accumulated apart from the small ones) -- relative RMS error of an output ~5e-8
 *            ... 7e-8 for K = 64 ... 128, a third of a K-long fp32 fmaf chain's; it is NOT bit-identical to such a chain
 *            (environment PCOPS_GEMM_BF3=0 selects the fp32 matrix pipe, which is).  An infinite input gives NaN (inf - inf
 *            in the split) where the chain gives inf; NaN stays NaN. */
int pcops_mlp_stats_rows(int M);
unsigned long long pcops_mlp_reduce_workspace_bytes(int N);
int pcops_mlp_gemm_fwd(int M, int K, int N, const float *X, int ldx, const float *pro_scale,
                       const float *pro_shift, const float *W, const float *bias, float *Y,
                       float *stats_partial, const float *stat_pivot, pcops_stream_t stream);
/* forward of a max-pooled LAST layer with the neighbourhood reduction (the reference's reduce_max over nsample,
 * pointnet_util.py:127) fused into the GEMM epilogue.  BN+ReLU is monotone per channel -- increasing for
 * gamma >= 0, decreasing for gamma < 0 (scale = gamma * rstd) -- so per group of S consecutive rows
 *   ysel[g,c] = max_s y (gamma[c] >= 0) | min_s y (gamma[c] < 0),  argsel[g,c] = first row attaining it (8 bit)
 * and, once scale/shift are known, pcops_mlp_pool_select gives out = relu(scale*ysel + shift) without re-reading
 * Y.  S % 32 == 0, S <= 256, M % S == 0, ldx == K -- or (round 5) groups that are NOT whole 32-row tiles: S % 4 == 0,
 * 8 <= S < 256, lcm(S, 32) <= 256 and M a multiple of it (DGCNN's T-Net: S = 20, MSG: S = 16; a wave walks lcm(S, 32)
 * rows = whole groups, a lane's four consecutive rows always lie inside one group; split-operand kernels only);
 * PCOPS_ERR_UNSUPPORTED when the shape is outside what pcops_mlp_gemm_fwd_pool_supported(M,K,N,S) accepts.
 * pro_scale == pro_shift == NULL: X is the stack's raw input.  Y == NULL: the activation is not stored at all (it then
 * only exists as statistics and group extrema) -- enough for a forward without backward and for the algebraic backward
 * of a pooled top layer below. */
int pcops_mlp_gemm_fwd_pool_supported(int M, int K, int N, int S);
int pcops_mlp_gemm_fwd_pool(int M, int K, int N, int S, const float *X, int ldx, const float *pro_scale,
                            const float *pro_shift, const float *W, const float *bias, const float *gamma,
                            float *Y, float *stats_partial, const float *stat_pivot, float *ysel,
                            unsigned char *argsel, pcops_stream_t stream);
int pcops_mlp_pool_select(long long G, int C, const float *ysel, const float *scale, const float *shift,
                          float *out, pcops_stream_t stream);
/* batch statistics -> mean, rstd = 1/sqrt(var+eps) (biased var), scale = gamma*rstd, shift = beta - mean*scale;
 * moving_* (may be NULL) <- decay*moving + (1-decay)*batch (unbiased batch variance if unbiased_moving_var).
 * P = rows of stats_partial, R = rows the statistics run over, workspace >= pcops_mlp_reduce_workspace_bytes(N).
 * stat_pivot: the pivot the producer of stats_partial was given (NULL: 0):  mean = pivot + s1/R,  var = s2/R - (s1/R)^2,
 * reduced and finalised in fp64.  stat_pivot may alias moving_mean (each channel reads it before its update). */
int pcops_mlp_bn_finalize(int P, int N, long long R, const float *stats_partial, const float *stat_pivot,
                          void *workspace, const float *gamma, const float *beta, float eps, float decay,
                          int unbiased_moving_var, float *moving_mean, float *moving_var, float *mean,
                          float *rstd, float *scale, float *shift, pcops_stream_t stream);
/* eval mode: scale/shift from the moving statistics */
int pcops_mlp_bn_eval_coeffs(int N, const float *gamma, const float *beta, const float *moving_mean,
                             const float *moving_var, float eps, float *scale, float *shift,
                             pcops_stream_t stream);
/* out[g,c] = max_s relu(scale[c]*Y[g*S+s,c] + shift[c]), argmax[g,c] (may be NULL) = first s attaining it,
 * ysel[g,c] (may be NULL) = Y at that row.  S<=256 */
int pcops_mlp_bn_relu_maxpool(long long G, int S, int C, const float *Y, const float *scale,
                              const float *shift, float *out, unsigned char *argmax, float *ysel,
                              pcops_stream_t stream);
/* out = relu(scale*Y + shift) (stack output without pooling) */
int pcops_mlp_bn_relu_apply(long long R, int C, const float *Y, const float *scale, const float *shift,
                            float *out, pcops_stream_t stream);
/* backward.  BN backward is folded into dY = p.G + q.Y + t with G = upstream grad masked by the ReLU.
 * relu_mask_stats: Gm = Gout*[relu(bn(Y))>0] and partial (sum Gm, sum Gm*Y): [pcops_mlp_bwd_stats_rows(R)][2][C]
 * pool_bwd_stats : the same sums for a max-pooled output, from (gpool, ysel = y at the pooled row): [..pool_stats_rows(G)][2][C];
 *                  gmasked (may be NULL) [G][C] = gpool * [relu(scale*ysel + shift) > 0], the MASKED pooled gradient --
 *                  this is what the `gpool` argument of pcops_mlp_gemm_dgrad* / pcops_mlp_wgrad* has to be: those kernels
 *                  place it at the arg-max rows without looking at the ReLU again (the wave-stream data gradient adds the
 *                  one row per (group, channel) AFTER staging the dense part q.Y + t -- one multiply-add per element
 *                  instead of byte extract, two compares, select and two multiply-adds)
 * bn_bwd_coeffs  : sums -> dgamma, dbeta, p, q, t */
int pcops_mlp_bwd_stats_rows(long long R);
int pcops_mlp_bwd_pool_stats_rows(long long G);
int pcops_mlp_relu_mask_stats(long long R, int C, const float *Gout, const float *Y, const float *scale,
                              const float *shift, float *Gm, float *stats_partial, pcops_stream_t stream);
int pcops_mlp_pool_bwd_stats(long long G, int C, const float *gpool, const float *ysel, const float *scale,
                             const float *shift, float *stats_partial, float *gmasked, pcops_stream_t stream);
/* ... of a pooled gradient that arrives as two pieces and / or with a row stride (an EdgeConv output that feeds the next layer AND a
 * column block of the concatenation, dgcnn/models/dgcnn.py:39-81): the sums of (ga + gb) -- gb may be NULL -- with rows lda / ldb
 * floats apart (multiples of 4, 16-byte aligned pointers), and gsum [G][C] = ga + gb, UNMASKED and contiguous, for the data-gradient
 * kernel behind (pcops_edge_pool_bwd*); round 6: autograd's sum of the two was a launch over the tensor, a strided piece a copy. */
int pcops_mlp_pool_bwd_stats_sum(long long G, int C, const float *ga, long long lda, const float *gb, long long ldb,
                                 const float *ysel, const float *scale, const float *shift, float *stats_partial,
                                 float *gsum, pcops_stream_t stream);
int pcops_mlp_bn_bwd_coeffs(int P, int N, long long R, const float *stats_partial, void *workspace,
                            const float *gamma, const float *mean, const float *rstd, float *dgamma,
                            float *dbeta, float *p, float *q, float *t, pcops_stream_t stream);
/* dgrad: Gprev[M,Nout] = mask . (dY[M,K] Wt[K,Nout]); dY from (G,Y,p,q,t) or, when gpool != NULL, from the
 * pooled form (gpool = the MASKED pooled gradient of pcops_mlp_pool_bwd_stats, argmax, S, pool_scale, pool_shift).
 * CONTRACT since ABI version 3: gpool must ALREADY carry the ReLU mask of the pooled rows (pass the `gmasked` output of
 * pcops_mlp_pool_bwd_stats, never the raw upstream gradient) -- the dgrad / wgrad / scatter kernels no longer test
 * relu(pool_scale * y + pool_shift) themselves; pool_scale / pool_shift are still REQUIRED non-NULL with a pooled form
 * (argument validation, and room to move the test back) but are not read.  A caller written against version 2 that passes
 * the raw gradient gets wrong gradients for inactive pooled rows: compare pcops_abi_version() first (the Python binding
 * refuses a mismatch, _lib.load()).
 * Yprev != NULL: mask = [relu(bn_prev(Yprev)) > 0]
 * and stats_partial [pcops_mlp_stats_rows(M)][2][Nout] gets (sum Gprev, sum Gprev*Yprev); Yprev == NULL: plain. */
int pcops_mlp_gemm_dgrad(int M, int K, int Nout, const float *G, const float *Y, const float *p,
                         const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                         int S, const float *pool_scale, const float *pool_shift, const float *Wt,
                         const float *Yprev, const float *prev_scale, const float *prev_shift, float *Gprev,
                         float *stats_partial, pcops_stream_t stream);
/* wgrad: dW[K,N] = A^T dY, db[N] (may be NULL) = 1^T dY; A = X or relu(X*a_scale + a_shift); dY as above.
 * partial: caller scratch of pcops_mlp_wgrad_splits(M,K,N) * (K*N + N) floats.
 * ARITHMETIC (round 4): layers wider than 64 on both sides with >= 32 768 rows are reduced on the bf16 matrix pipe with
 * split operands (three bf16 pieces per fp32 value, six exact partial products, the large ones accumulated apart from the
 * small ones): fp32 in, fp32 out, 1.5e-7 ... 2.2e-7 relative RMS against float64 where the fp32-pipe kernel makes
 * 2.1e-7 ... 4.0e-7; not bit-identical to it (environment PCOPS_WGRAD_BF3=0 selects the fp32 pipe). */
int pcops_mlp_wgrad_splits(long long M, int K, int N);
int pcops_mlp_wgrad(long long M, int K, int N, const float *X, int ldx, const float *a_scale,
                    const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                    const float *t, const float *gpool, const unsigned char *argmax, int S,
                    const float *pool_scale, const float *pool_shift, float *partial, float *dW, float *db,
                    pcops_stream_t stream);
int pcops_mlp_transpose(int K, int N, const float *W, float *Wt, pcops_stream_t stream);
/* Data AND weight gradient of a narrow layer in one pass (round 3): what pcops_mlp_gemm_dgrad (with Yprev) followed by
 * pcops_mlp_wgrad (A = relu(Yprev*a_scale + a_shift)) compute for the layer  Y = relu(bn(Yprev)) W + b,  W [K][N] in its
 * own layout (no transposed copy), with every tensor read ONCE.  The 64-wide layers of the reference's stacks are
 * bandwidth bound in both kernels and read the same bytes twice.
 *   pcops_mlp_bwd_fused_groups  0 when (M, K, N, S, pooled) is not taken (K <= 64, N <= 128, M >= 65536, both % 4 == 0);
 *                               otherwise the number of partial copies: partial = groups * (K N + N) floats,
 *                               stats_partial [groups][2][K] = (sum Gprev, sum Gprev*Yprev) -- the partial-row count to
 *                               hand to pcops_mlp_bn_bwd_coeffs
 *   G / Y / p / q / t / gpool / argmax / S   as pcops_mlp_gemm_dgrad
 * Same numbers as the two-kernel path up to rounding; sums in a fixed order (deterministic).  ARITHMETIC (round 4): the
 * data gradient dX = dY W^T is evaluated on the bf16 matrix pipe with split operands (three bf16 pieces per fp32 value,
 * six exact partial products, the large ones accumulated apart from the small ones): fp32 in, fp32 out, no less accurate
 * than the fp32 chain, not bit-identical to it (environment PCOPS_BWD_FUSED_DX3=0 selects the fp32 pipe); the weight
 * gradient half runs on the fp32 pipe -- round 6: on the bf16 pipe as well, from transposed pieces the staging waves split
 * (option value 2, the default), for 65..128 output columns over rows that are read (not the xyz form). */
int pcops_mlp_bwd_fused_groups(long long M, int K, int N, int S, int pooled);
int pcops_mlp_bwd_fused(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                        const float *G, const float *Y, const float *p, const float *q, const float *t,
                        const float *gpool, const unsigned char *argmax, int S, const float *W, float *partial,
                        float *dW, float *db, float *Gprev, float *stats_partial, pcops_stream_t stream);
/* ... over compacted rows (pcops_rows_t; M = the allocated row count, as for the other _rows entry points) */
int pcops_mlp_bwd_fused_rows(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                             const float *G, const float *Y, const float *p, const float *q, const float *t,
                             const float *gpool, const unsigned char *argmax, int S, const float *W, float *partial,
                             float *dW, float *db, float *Gprev, float *stats_partial, const pcops_rows_t *rows,
                             pcops_stream_t stream);
/* out [M][N] = (t + p.G) + q.Y row by row (N % 4 == 0, 16-byte aligned pointers; p / q / t [N]): the BatchNorm-backward
 * combination dY = p.G + q.Y + t as a tensor -- the data gradient of a first layer whose gather is the identity (the
 * whole-cloud group of sample_and_group_all, pointnet_util.py:59-84), where no scatter kernel is needed to form it. */
int pcops_mlp_dy_apply(long long M, int N, const float *G, const float *Y, const float *p, const float *q, const float *t,
                       float *out, pcops_stream_t stream);
/* C [M][N] = A [M][K] B [K][N], row-major with leading dimensions: the small weight x weight products and row vectors
 * around the big kernels (32 x 32 output tile per workgroup, fp32 MFMA, fixed summation order) */
int pcops_small_gemm(int M, int K, int N, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                     pcops_stream_t stream);
/* C = op(A) op(B) + bias: transA != 0 -> A is stored [K][M], transB != 0 -> B is stored [N][K]; bias [N] or NULL.
 * The three products of a fully connected layer on a few hundred rows (tf_util.py:187-213 fully_connected: Y = X W + b,
 * dX = dY W^T, dW = X^T dY) without a transposed copy of anything. */
int pcops_small_gemm_ex(int M, int K, int N, const float *A, int lda, int transA, const float *B, int ldb, int transB,
                        const float *bias, float *C, int ldc, pcops_stream_t stream);
/* ... and colsum [N] (may be NULL) = the column sums of op(B) over its K rows out of the same launch: the bias gradient
 * db = 1^T dY of fully_connected next to dW = X^T dY (tf_util.py:187-213; round 6 -- it was a separate reduction launch
 * of 12 us per layer).  Fixed summation order. */
int pcops_small_gemm_colsum(int M, int K, int N, const float *A, int lda, int transA, const float *B, int ldb, int transB,
                            const float *bias, float *C, int ldc, float *colsum, pcops_stream_t stream);
/* TWO independent products of that form in ONE launch -- p[0] and p[1]: the data and the weight gradient of a fully connected
 * layer (dX = dY W^T, dW = X^T dY with db as colsum), which share dY and each fill half the chip when launched alone; the
 * two K x K / K x N products of the algebraic top layer.  Same results as two pcops_small_gemm_colsum calls, bit for bit. */
typedef struct pcops_gemm_problem {
    int M, K, N;
    const float *A; int lda, transA;
    const float *B; int ldb, transB;
    const float *bias;              /* [N] or NULL */
    float *C; int ldc;
    float *colsum;                  /* [N] or NULL */
} pcops_gemm_problem_t;
int pcops_small_gemm_pair(const pcops_gemm_problem_t *p, pcops_stream_t stream);

/* ---- algebraic backward of a POOLED top layer (the last conv of a set-abstraction stack / of a stack pooled over a
 * whole cloud: pointnet_util.py:139-147, dgcnn.py "agg", transform_nets.py "tconv3").
 *   Y = X W + b,  X = relu(bn_prev(Yprev)) [M][Kp],  out[g] = max over the S rows of group g of relu(bn(Y))
 * dY = p.G + q.Y + t has ONE non-zero row of G per (group, channel).  Substituting Y = X W + b:
 *   dX = X (W diag(q) W^T) + 1 (W (q.b + t))^T + (p.G) W^T            Kp x Kp product instead of N x Kp
 *   dW = (X^T X) (W diag(q)) + (X^T 1)(q.b + t)^T + X^T (p.G)         Kp x Kp Gram matrix instead of Kp x N
 *   db = 1^T (p.G) + q.((X^T 1) W + M b) + M t
 * Neither needs Y; the (p.G) terms touch M/S * N rows.  N = 2 Kp .. 8 Kp in the reference's stacks, so the two large
 * products lose 1/2 .. 7/8 of their flops.  Same numbers as pcops_mlp_gemm_dgrad / pcops_mlp_wgrad up to fp32
 * rounding (different summation order).
 *   pcops_mlp_pool_top_supported  1 when the four entry points below take (M, Kp, N, S)
 *   pcops_mlp_pool_top_addend       addend [(M/S) min(S,N)][Kp] = the rows of (p.G) W^T that are not zero, compacted;
 *                                 rowmap [M] = slot of a row or -1.  gout / ysel / argmax [M/S][N] as in
 *                                 pcops_mlp_gemm_dgrad (gpool form), Wt [N][Kp] from pcops_mlp_transpose
 *   pcops_mlp_gemm_dgrad_top      Gprev [M][Kp] = mask_prev . (X Mq + addend[rowmap] + vconst), stats_partial as
 *                                 pcops_mlp_gemm_dgrad;  Mq [Kp][Kp] = W diag(q) W^T, vconst [Kp] = W (q.b + t)
 *   pcops_mlp_gram                gram [Kp][Kp] = X^T X, xsum [Kp] = X^T 1; partial: pcops_mlp_wgrad_splits(M,Kp,Kp)
 *                                 copies of (Kp Kp + Kp) floats
 *   pcops_mlp_pool_top_wsparse    Ssp [Kp][N] = X^T (p.G), cfsum [N] = 1^T (p.G)
 *   pcops_mlp_pool_top_prep       the small operands in one launch: Wt [N][Kp] = W^T, Wq [Kp][N] = W diag(q),
 *                                 u [N] = q.b + t, v [Kp] = W u (= vconst; v may be NULL)  (round 6: they were a transpose,
 *                                 two elementwise launches and a matrix-vector launch)
 *   pcops_mlp_pool_top_finish     closes the sums in place: dW [Kp][N] = (dW + Ssp) + xsum u^T with dW = gram Wq on
 *                                 entry, db [N] = (cfsum + q.(xsum^T W + M b)) + M t  (round 6: eleven launches)
 * prev_scale == prev_shift == NULL: X is the stack's raw input (a one-layer stack) -- no mask, no statistics.
 * All sums in a fixed order (deterministic). */
int pcops_mlp_pool_top_supported(int M, int Kp, int N, int S);
int pcops_mlp_pool_top_prep(int Kp, int N, const float *W, const float *b, const float *q, const float *t, float *Wt,
                            float *Wq, float *u, float *v, pcops_stream_t stream);
int pcops_mlp_pool_top_finish(int Kp, int N, long long M, float *dW, const float *Ssp, const float *xsum, const float *u,
                              const float *cfsum, const float *q, const float *W, const float *b, const float *t,
                              float *db, pcops_stream_t stream);
int pcops_mlp_pool_top_addend(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                            const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                            const float *p, const float *Wt, float *addend, int *rowmap, pcops_stream_t stream);
int pcops_mlp_gemm_dgrad_top(int M, int Kp, const float *Yprev, const float *prev_scale, const float *prev_shift,
                             const float *Mq, const float *vconst, const float *addend, long long addend_rows,
                             const int *rowmap, float *Gprev, float *stats_partial, pcops_stream_t stream);
int pcops_mlp_gram(long long M, int Kp, const float *Yprev, int ldx, const float *a_scale, const float *a_shift,
                   float *partial, float *gram, float *xsum, pcops_stream_t stream);
int pcops_mlp_pool_top_wsparse(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                               const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                               const float *p, const float *Yprev, const float *prev_scale, const float *prev_shift,
                               float *Ssp, float *cfsum, pcops_stream_t stream);
/* ... for MANY SMALL groups on uncompacted rows (S = 32 / 64 with N = 128: nearly every row is some channel's arg-max, a
 * compact addend would be as large as X).  The sparse halves stay on the chip, each call is ONE pass over Yprev:
 *   pcops_mlp_dgrad_top_groups   Gprev [M][Kp] = mask_prev . (X Mq + vconst + sum_c cf[g,c] Wt[c,:] on row argmax[g,c]),
 *                                cf = p gout where pool_scale ysel + pool_shift > 0, else 0 (pcops_mlp_pool_top_addend's
 *                                coefficient); stats_partial [pcops_mlp_stats_rows(M)][2][Kp] as pcops_mlp_gemm_dgrad_top
 *   pcops_mlp_wgrad_top_groups   gram = X^T X (full, mirrored), xsum = X^T 1, Ssp [Kp][N] = X^T (p.G), cfsum [N] = 1^T (p.G):
 *                                what pcops_mlp_gram + pcops_mlp_pool_top_wsparse give; partial: scratch of
 *                                pcops_mlp_pool_top_groups_partial(M, Kp, N) floats (a copy of Kp Kp + Kp + Kp N + N per
 *                                workgroup)
 * prep, the small products and finish are the ones above.  Both take Kp == 64, N % 32 == 0 with 2 Kp <= N <= 256, S = 32 or
 * 64, M % S == 0, M Kp 4 below the 32-bit bound of the calls above, 16-byte aligned rows; PCOPS_ERR_UNSUPPORTED otherwise,
 * before any pointer check.  prev_scale / prev_shift are required.  pcops_mlp_pool_top_groups_supported is the ONE answer a
 * planner asks: that shape AND M >= 262144 (below it the Y this form does not store stays in the cache level; a planning
 * threshold, not a kernel limit).  No float atomics, every sum in a fixed order. */
int pcops_mlp_pool_top_groups_supported(int M, int Kp, int N, int S);
int pcops_mlp_pool_top_groups_partial(int M, int Kp, int N);
int pcops_mlp_dgrad_top_groups(int M, int Kp, int N, int S, const float *Yprev, const float *prev_scale,
                               const float *prev_shift, const float *Mq, const float *vconst, const float *gout,
                               const float *ysel, const unsigned char *argmax, const float *pool_scale,
                               const float *pool_shift, const float *p, const float *Wt, float *Gprev, float *stats_partial,
                               pcops_stream_t stream);
int pcops_mlp_wgrad_top_groups(int M, int Kp, int N, int S, const float *Yprev, const float *prev_scale,
                               const float *prev_shift, const float *gout, const float *ysel, const unsigned char *argmax,
                               const float *pool_scale, const float *pool_shift, const float *p, float *partial, float *gram,
                               float *xsum, float *Ssp, float *cfsum, pcops_stream_t stream);
/* The layer that FOLLOWS an arithmetic first layer  y1[row][k] = fma(dz, w2[k], fma(dy, w1[k], fma(dx, w0[k], b[k])))
 * (grouped xyz offsets only: the first set-abstraction level, pointnet_util.py:44-54 with points == None).  y1 is
 * rebuilt from off4 [M][4] = (dx, dy, dz, 0) and xyzw [4][C1] (rows w0, w1, w2, b) wherever the plain entry points
 * would read it -- as the forward operand, as the weight gradient's A side, and in the data gradient's ReLU mask and
 * BN-backward statistics -- so the (rows, C1) first-layer tensor never exists.  Same arguments as the plain
 * functions otherwise.  Wave-stream shapes only: check pcops_mlp_xyz_supported(M, C1, N2) first
 * (PCOPS_ERR_UNSUPPORTED otherwise).
 * pcops_mlp_gemm_dgrad_xyz: xyz_stats (may be NULL) = float [pcops_mlp_stats_rows(M)][3][Nout] partial sums of
 * off[row][i] * Gprev[row][c].  The first layer's gradients are LINEAR in a handful of such sums,
 *   dWxyz[i][c] = p[c] A[i][c] + q[c] B[i][c] + t[c] S[i],   dbias[c] = p[c] sumG[c] + q[c] sumY[c] + t[c] rows
 * (A = these sums, sumG / sumGY = stats_partial, B = M33 Wxyz + S^T b and S from the offset moments the forward
 * gather emits), so with xyz_stats Gprev may be NULL: the (rows, C1) gradient is neither written nor scattered. */
int pcops_mlp_xyz_supported(int M, int C1, int N2);
/* pcops_mlp_bwd_fused over the xyz form (round 3): pcops_mlp_wgrad_xyz + pcops_mlp_gemm_dgrad_xyz (Gprev == NULL form) in
 * one pass -- dW, db of the layer, stats_partial [groups][2][K] and xyz_stats [groups][3][K] of the arithmetic layer
 * below; groups = pcops_mlp_bwd_fused_groups(M, K, N, S, pooled), 0 = not taken.  W [K][N] as the forward holds it.
 * K == N == 64 with rows == NULL and gpool == NULL (M * 256 bytes below 2^31) takes the all-wave tile kernel of
 * csrc/xyz_bwd_tiles.hip, both products on split bf16 operands (pcops_last_launch_pipe() 1, plan path 17); same buffers,
 * same sizes.  PCOPS_BWD_XYZ_TILES=0 in the environment, read once by the library, gives bwd_fused_kernel back for every shape. */
int pcops_mlp_bwd_fused_xyz_rows(long long M, int K, int N, const float *off4, const float *xyzw, const float *a_scale,
                                 const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                                 const float *t, const float *gpool, const unsigned char *argmax, int S, const float *W,
                                 float *partial, float *dW, float *db, float *stats_partial, float *xyz_stats,
                                 const pcops_rows_t *rows, pcops_stream_t stream);
/* The one-pass backward of a 128 -> 128 layer whose input rows are read (csrc/bwd_tiles128.hip): what
 * pcops_mlp_gemm_dgrad_rows (with Yprev) followed by pcops_mlp_wgrad_rows compute for  Y = relu(bn(Yprev)) W + b,  every tensor
 * read once -- Gprev [M][K] = mask . (dY W^T), stats_partial [groups][2][K] = (sum Gprev, sum Gprev Yprev), dW, db.  Both
 * products run on the bf16 matrix pipe with split operands (six products, large and small terms in separate accumulators;
 * pcops_last_launch_pipe() 1, plan path 18 with [1] = 2, [2] = 128, [4] = 4 over compacted rows).  No float atomics: the
 * workgroups' partial copies are added in a fixed order, two calls give the same bits, deterministic mode takes the same kernel.
 *   pcops_mlp_bwd_tiles_groups  the launcher's own answer: 0 when (M, K, N) is not taken (K == N == 128, 64 <= M, M * 512 bytes
 *                               below 2^31), otherwise the number of partial copies: partial = groups * (K N + N) floats,
 *                               stats_partial rows = groups.  PCOPS_BWD_TILES128=0 in the environment, read once by the
 *                               library, makes it answer 0 for every shape.  pcops_mlp_bwd_fused_groups is not affected.
 *   rows  NULL or a compacted row set (M = the allocated row count): the row that opens a block has dY = p.G + w (q.Y + t)
 *         with the block's weight w, exactly as the two _rows entry points above form it; Gprev rows past the device row
 *         count are not written.  Yprev, G, Y, W, Gprev 16-byte aligned (else PCOPS_ERR_UNSUPPORTED). */
int pcops_mlp_bwd_tiles_groups(long long M, int K, int N);
int pcops_mlp_bwd_tiles_rows(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                             const float *G, const float *Y, const float *p, const float *q, const float *t, const float *W,
                             float *partial, float *dW, float *db, float *Gprev, float *stats_partial, const pcops_rows_t *rows,
                             pcops_stream_t stream);
int pcops_mlp_gemm_fwd_xyz(int M, int K, int N, const float *off4, const float *xyzw, const float *pro_scale,
                           const float *pro_shift, const float *W, const float *bias, float *Y,
                           float *stats_partial, const float *stat_pivot, pcops_stream_t stream);
int pcops_mlp_gemm_dgrad_xyz(int M, int K, int Nout, const float *G, const float *Y, const float *p,
                             const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                             int S, const float *pool_scale, const float *pool_shift, const float *Wt,
                             const float *off4, const float *xyzw, const float *prev_scale,
                             const float *prev_shift, float *Gprev, float *stats_partial, float *xyz_stats,
                             pcops_stream_t stream);
int pcops_mlp_wgrad_xyz(long long M, int K, int N, const float *off4, const float *xyzw, const float *a_scale,
                        const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                        const float *t, const float *gpool, const unsigned char *argmax, int S,
                        const float *pool_scale, const float *pool_shift, float *partial, float *dW, float *db,
                        pcops_stream_t stream);

/* --------------------------------------------- first grouped layer in front of the grouping (gather.hip)
 * A 1x1 conv is linear: concat(xyz[idx] - new_xyz, points[idx]) W = (points W_f)[idx] + (xyz[idx] - new_xyz) W_xyz
 * (pointnet2/utils/pointnet_util.py:44-54,117-122; EdgeConv concat(x_i, x_j - x_i): dgcnn/utils/tf_util.py:699-705
 * + dgcnn.py:39-44), so the feature contraction runs once per SOURCE point and the (b,m,s,c) activation is
 *     Y[b,j,s,:] = Q[b, idx[b,j,s], :] + Ctr[b,j,:] + (xyz[b,idx,:] - new_xyz[b,j,:]) Wxyz + bias
 * Q (b,n,c), Ctr (b,m,c), xyz (b,n,3), new_xyz (b,m,3), Wxyz (3,c), bias (c), idx (b,m,s); Q, Ctr, the coordinate
 * term and bias are each optional (NULL); the coordinate term is evaluated on the centred offsets (no cancellation).
 * stats_partial (may be NULL): float [pcops_sa_gather_stats_rows(b*m)][2][c] partial sums of (Y - pivot) and
 * (Y - pivot)^2, pivot = stat_pivot [c] or 0 (shifted moments, see pcops_mlp_gemm_fwd).
 * Y may be NULL (statistics only) and off4 (may be NULL; needs the coordinate term) receives the centred offsets
 * (dx, dy, dz, 0) per grouped row, float [b*m*s][4]: when the layer has NO Q / Ctr term it is arithmetic in those
 * three numbers, and the pcops_mlp_*_xyz entry points rebuild it on the fly instead of reading a (b,m,s,c) tensor.
 * moments (may be NULL; needs the coordinate term): float [pcops_sa_gather_stats_rows(b*m)][9] partial sums of
 * (dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz) -- see pcops_mlp_gemm_dgrad_xyz.
 * With Q, Ctr and Y all NULL and moments given, y_c = w_c . o + bias_c, and the statistics are taken from the moments
 * (M1 = sum o, M2 = sum o o^T, R rows):  sum (y_c - pv_c) = w_c . M1 + R (bias_c - pv_c),  sum (y_c - pv_c)^2 =
 * w_c^T M2 w_c + 2 (bias_c - pv_c) w_c . M1 + R (bias_c - pv_c)^2, formed in double and written as row 0 of stats_partial,
 * the other rows zero (PCOPS_OPT_XYZ_STATS_MOMENTS = 1; the default 0 sums over the rebuilt outputs as in every other form). */
int pcops_sa_gather_stats_rows(long long groups);
/* rows of stats_partial a pcops_sa_gather_fwd(_rows) call of this form writes: the Q + Ctr form with a stored Y runs on
 * the 64-channel-slice kernel of csrc/edgeconv.hip (one row per 64 groups) when the shape fits; everything else writes
 * pcops_sa_gather_stats_rows(b*m) rows.  has_q / has_ctr: the term is present; other_terms: any of Wxyz, bias, off4,
 * moments; compacted: a pcops_rows_t is passed. */
int pcops_sa_gather_fwd_stats_rows(int b, int n, int m, int s, int c, int has_q, int has_ctr, int other_terms,
                                   int compacted);
int pcops_sa_gather_fwd(int b, int n, int m, int s, int c, const float *Q, const float *Ctr, const float *xyz,
                        const float *new_xyz, const float *Wxyz, const float *bias, const int *idx, float *Y,
                        float *off4, float *stats_partial, const float *stat_pivot, float *moments,
                        pcops_stream_t stream);
/* backward through the BN+ReLU that follows: dY = p.G + q.Y + t (pooled form when gpool != NULL, as in
 * pcops_mlp_gemm_dgrad).  Outputs, each optional: dQ (b,n,c) = scatter-add of dY over idx (zeroed here),
 * dCtr (b,m,c) = sum over s, dWxyz (3,c) = sum (xyz[idx]-new_xyz)^T dY (needs xyz/new_xyz), dbias (c) = sum dY.
 * wpartial: caller scratch of pcops_sa_scatter_rows(b, m) * 4 * c floats (needed for dWxyz / dbias).
 * fwd_Q / fwd_Ctr / fwd_Wxyz / fwd_bias (all may be NULL): the arguments pcops_sa_gather_fwd was called with.  When
 * the forward had no Q / Ctr term (Y = (xyz[idx]-new_xyz) Wxyz + bias) the streaming kernel REBUILDS Y in the
 * forward's own operation order instead of reading it (bit-identical, one (b,m,s,c) tensor less to stream); Y may
 * be NULL only in that case with dQ == NULL.
 * With fwd_Q != NULL and fwd_Ctr == NULL the chunked walk below (G materialised, workspace given, no dCtr, not
 * deterministic) uses them too: Y[r] = fwd_Q[idx] + offsets fwd_Wxyz + fwd_bias, so the sums over a point's rows are
 *     dQ[i] = p.sum G + q.(W_i (Q[i] + bias) + Wxyz^T O_i) + W_i t,   W_i = sum of the row weights, O_i = sum weight * offset
 * and dWxyz / dbias follow from the same sums and nine global offset moments -- the rows of Y are not read (they must
 * still be the forward's: PCOPS_OPT_SCATTER_QFORM = 0 reads them, and both forms agree to fp32 summation order).
 * workspace (may be NULL): pcops_sa_scatter_workspace_bytes(b,n,m,s) bytes, 16-byte aligned; with it the feature
 * gradient is computed as a GATHER over a per-cloud inverse index (counting sort of idx) -- one wave per source
 * point, no float atomics; without it (or when dCtr / the pooled form is requested) dQ is accumulated with atomics
 * in an LDS-resident slice per cloud. */
int pcops_sa_scatter_rows(int b, int m);
unsigned long long pcops_sa_scatter_workspace_bytes(int b, int n, int m, int s);
int pcops_sa_scatter_bwd(int b, int n, int m, int s, int c, const float *G, const float *Y, const float *p,
                         const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                         const float *pool_scale, const float *pool_shift, const int *idx, const float *xyz,
                         const float *new_xyz, float *dQ, float *dCtr, float *wpartial, float *dWxyz,
                         float *dbias, const float *fwd_Q, const float *fwd_Ctr, const float *fwd_Wxyz,
                         const float *fwd_bias, void *workspace, pcops_stream_t stream);

/* EdgeConv as ONE pooled layer without the (b,n,k,c) tensor in either direction (dgcnn/models/dgcnn.py:39-48 with the
 * first-layer restructuring above):  y[g,s,:] = Q[idx[g,s],:] + Ctr[g,:] -> BN -> ReLU -> max over s.  Ctr is constant
 * inside a group and BN+ReLU is monotone per channel, so
 *   forward : qsel[g,c] = max_s (gamma[c] >= 0) | min_s (gamma[c] < 0) of Q[idx[g,s],c], arg = first s attaining it,
 *             SQ[g,c] = sum_s Q[idx[g,s],c];  stats_partial [pcops_edge_pool_fwd_stats_rows(b,n,m,s,c)][2][c] = partial
 *             (sum y', sum y'^2), y' = y - stat_pivot (shifted moments, see pcops_mlp_gemm_fwd), evaluated as
 *             (SQ' + k c', SQ2' + 2 c' SQ' + k c'^2) with Q taken relative to its own first row, q' = q - Q[0,0,:], and
 *             c' = Ctr + Q[0,0,:] - pivot, so that neither a common offset of Q nor one of Ctr cancels in fp32
 *             -> pcops_mlp_bn_finalize with the same pivot
 *   out     : out = relu(scale (qsel + Ctr) + shift), ysel = qsel + Ctr
 *   backward: with (p, q, t) from pcops_mlp_pool_bwd_stats(gpool, ysel) + pcops_mlp_bn_bwd_coeffs,
 *             dCtr[g] = q (SQ + k Ctr) + k t + a[g],  a = p gpool [relu(bn(ysel)) > 0],
 *             dQ[i] = cnt_i (q Q[i] + t) + q sum_{(g,s)->i} Ctr[g] + sum_{g: arg row -> i} a[g]   (inverse index of idx)
 * workspace: pcops_sa_scatter_workspace_bytes(b,n,m,s) bytes.  s <= 256. */
int pcops_edge_pool_stats_rows(long long groups);     /* ABI >= 4: an UPPER BOUND (buffer size) only, see below */
/* ABI version 4 (round 6, was an unversioned change of round 5): pcops_edge_pool_fwd and pcops_sa_gather_fwd write the number
 * of rows THESE per-shape queries return -- rows beyond stay untouched -- so pcops_mlp_bn_finalize must be given that count,
 * not the shape-less one; a caller built against the round-4 header must be rebuilt (pcops_abi_version() tells).
 * rows of stats_partial THIS call shape writes (<= pcops_edge_pool_stats_rows(b*m)): the 64-channel-slice kernels of
 * csrc/edgeconv.hip write one row per 64 groups, or one per cloud when the cloud's slice is LDS-resident */
int pcops_edge_pool_fwd_stats_rows(int b, int n, int m, int s, int c);
int pcops_edge_pool_fwd(int b, int n, int m, int s, int c, const float *Q, const float *Ctr, const int *idx,
                        const float *gamma, float *SQ, float *qsel, unsigned char *arg, float *stats_partial,
                        const float *stat_pivot, pcops_stream_t stream);
int pcops_edge_pool_out(long long groups, int c, const float *qsel, const float *Ctr, const float *scale,
                        const float *shift, float *out, float *ysel, pcops_stream_t stream);
int pcops_edge_pool_bwd(int b, int n, int m, int s, int c, const float *Q, const float *Ctr, const int *idx,
                        const float *gpool, const float *ysel, const float *SQ, const unsigned char *arg,
                        const float *scale, const float *shift, const float *p, const float *q, const float *t,
                        float *dQ, float *dCtr, void *workspace, pcops_stream_t stream);
/* First layer of a stack whose groups are WHOLE CLOUDS in their own row order (round 5; reference: dgcnn_bga.py:118-128, the
 * segmentation head's concat of 1280 per-cloud channels with 320 per-point ones -- see DESIGN.md section 4.15):
 *   Y[r, :] = Q[r, :] + Ctr[r / rows_per_group, :]  with shifted-moment partials [pcops_cloud_bias_rows(rows)][2][c], and
 *   backward  dQ = p G + q Y + t  (may be NULL),  dCtr[g] = sum over the group's rows of it; partial: [..rows(rows)][c] scratch.
 * rows_per_group a multiple of 256, c % 4 == 0, c <= 1024, 256 % (c / 4) == 0.  The general form of the same layer is
 * pcops_sa_gather_fwd / pcops_sa_scatter_bwd with the identity index. */
int pcops_cloud_bias_supported(long long rows, int rows_per_group, int c);
int pcops_cloud_bias_rows(long long rows);
int pcops_cloud_bias_fwd(long long rows, int rows_per_group, int c, const float *Q, const float *Ctr, float *Y,
                         float *stats_partial, const float *stat_pivot, pcops_stream_t stream);
int pcops_cloud_bias_bwd(long long rows, int rows_per_group, int c, const float *G, const float *Y, const float *p, const float *q,
                         const float *t, float *dQ, float *dCtr, float *partial, pcops_stream_t stream);
/* First EdgeConv layer of a grouped stack whose INPUT needs no gradient (round 5; reference: the T-Net's tconv1 on the edge
 * features of the raw cloud, dgcnn/models/transform_nets.py:18-27 over tf_util.get_edge_feature, tf_util.py:660-706).  The
 * layer is linear in the six edge channels e = [x_g | x_j - x_g], j = idx[g, s]:  Y1 = e W + b, and with the BN backward
 * dY1 = p Gm + q Y1 + t of the layer
 *   dW (6, c) = p (E^T Gm) + q (E^T E W + E^T 1 b) + t E^T 1,     db = p sum Gm + q sum Y1 + t rows
 * -- one streaming pass over the masked gradient Gm (b m s, c) instead of the scatter to per-point gradients
 * (pcops_sa_scatter_bwd_ld: two passes over Gm, one a gather through an inverse index) and the GEMM backward behind it.
 *   pcops_edge_first_moments: moments_partial [pcops_edge_first_rows()][27] -- 21 second moments of e (upper triangle,
 *     row-major) then its 6 sums; forward time (xyz (b, n, 3), idx (b, m, s), m == n for an EdgeConv graph); edge_rows
 *     (may be NULL): the rows e themselves, (b m s, 8) with two pad floats, for pcops_mlp_bwd_fused_edge;
 *   pcops_edge_first_wgrad:   wpartial [pcops_edge_first_rows()][6][c] = partial sums of E^T Gm (c = 64 | 128);
 *   pcops_edge_first_layer_grads: dW (6, c), dbias (c, may be NULL) from both, p / q / t and sumG (= dbeta) from
 *     pcops_mlp_bn_bwd_coeffs, mean from pcops_mlp_bn_finalize, rows = b m s; sums in double, fixed order. */
int pcops_edge_first_rows(void);
int pcops_edge_first_supported(int b, int n, int m, int s, int c);
int pcops_edge_first_moments(int b, int n, int m, int s, const float *xyz, const int *idx, float *moments_partial,
                             float *edge_rows, pcops_stream_t stream);
int pcops_edge_first_wgrad(int b, int n, int m, int s, int c, const float *G, const float *xyz, const int *idx,
                           float *wpartial, pcops_stream_t stream);
/* the one-pass backward (pcops_mlp_bwd_fused_rows) of the POOLED layer above such a first layer: the masked gradient of
 * the first layer is not written -- E^T Gm leaves as edge_stats [pcops_mlp_bwd_fused_edge_groups(M, K, N, S, 0)][6][K], in
 * the place of pcops_edge_first_wgrad's wpartial.  Groups of S rows that are not whole 32-row tiles (the k neighbours).
 *   pcops_mlp_bwd_fused_edge_groups  the edge forms' own query: 0 when pcops_mlp_bwd_fused_edge (gram = 0) or
 *                                    pcops_mlp_bwd_fused_edge_gw (gram = 1) does not take (M, K, N, S), otherwise the
 *                                    partial copies -- pcops_mlp_bwd_fused_groups / _gw_groups with S % 32 == 0 refused */
int pcops_mlp_bwd_fused_edge_groups(long long M, int K, int N, int S, int gram);
int pcops_mlp_bwd_fused_edge(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                                  const float *Y, const float *p, const float *q, const float *t, const float *gpool,
                                  const unsigned char *argmax, int S, const float *W, float *partial, float *dW, float *db,
                                  float *stats_partial, const float *edge_rows, float *edge_stats, pcops_stream_t stream);

/* Round 6: pcops_mlp_bwd_fused / pcops_mlp_bwd_fused_edge of a POOLED layer with the weight gradient in its GRAM FORM.  With
 * dY = p.G + q.Y + t, one non-zero row of G per (group, channel), and Y = X W + bias:
 *     dW = X^T (p.G) + (X^T X) W diag(q) + (X^T 1)(q.bias + t)^T
 * -- a 64 x 64 Gram matrix on the matrix pipe instead of the K x N product (half the weight gradient's matrix time at
 * N = 128), the arg rows as vector work, the K x N product once on the summed partials.  Same reference op as
 * pcops_mlp_bwd_fused (tf.gradients of conv2d + batch_norm + reduce_max, pointnet2/utils/pointnet_util.py:117-127,
 * dgcnn/models/transform_nets.py:19-27); results equal to it to fp32 rounding.  Uncompacted rows, 11 <= S <= 255
 * (whole 32-row tiles included; the edge form: S % 32 != 0 only, pcops_mlp_bwd_fused_edge_groups(M, K, N, S, 1)),
 * PCOPS_OPT_BWD_FUSED_DX_SPLIT_BF16 on; bias [N] may be NULL (a layer without bias).
 *   pcops_mlp_bwd_fused_gw_groups  workgroups = partial copies, 0 when the shape is not taken
 *   partial: groups (K N + N + K K + K) floats of scratch */
int pcops_mlp_bwd_fused_gw_groups(long long M, int K, int N, int S);
int pcops_mlp_bwd_fused_gw(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                           const float *Y, const float *p, const float *q, const float *t, const float *gpool,
                           const unsigned char *argmax, int S, const float *W, const float *bias, float *partial, float *dW,
                           float *db, float *Gprev, float *stats_partial, pcops_stream_t stream);
int pcops_mlp_bwd_fused_edge_gw(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                                const float *Y, const float *p, const float *q, const float *t, const float *gpool,
                                const unsigned char *argmax, int S, const float *W, const float *bias, float *partial,
                                float *dW, float *db, float *stats_partial, const float *edge_rows, float *edge_stats,
                                pcops_stream_t stream);
int pcops_edge_first_layer_grads(int P1, const float *wpartial, int P2, const float *moments_partial, int c, const float *W,
                                 const float *bias, const float *p, const float *q, const float *t, const float *sumG,
                                 const float *mean, long long rows, float *dW, float *dbias, pcops_stream_t stream);
/* dWxyz (3,c) and dbias (c, may be NULL) of an arithmetic first layer from the sums described at
 * pcops_mlp_gemm_dgrad_xyz: xyz_stats [P1][3][c], moments [P2][9] (pcops_sa_gather_fwd), p/q/t and sumG (= dbeta) from
 * pcops_mlp_bn_bwd_coeffs, mean from pcops_mlp_bn_finalize, rows = b*m*s. */
int pcops_xyz_first_layer_grads(int P1, const float *xyz_stats, int P2, const float *moments, int C,
                                const float *Wxyz, const float *bias, const float *p, const float *q, const float *t,
                                const float *sumG, const float *mean, long long rows, float *dWxyz, float *dbias,
                                pcops_stream_t stream);

/* ------------------------------------------------------------------ compacted rows
 * query_ball_point pads a neighbourhood that holds fewer than nsample points with copies of its first member
 * (grouping/tf_grouping_g.cu:26-32), and the reference pushes every copy through the whole shared MLP
 * (pointnet2/utils/pointnet_util.py:117-127): at the PB_T50_RS-shaped SSG config 39 % of the rows of the second
 * set-abstraction level are such copies.  A copy computes exactly what its original computes, so the grouped stack
 * runs on a COMPACTED row set instead -- per group its pts_cnt real members, rounded up to whole blocks of 16 rows
 * with copies of member 0 (16 * ceil(cnt / 16) <= nsample rows instead of nsample) -- and the first row of every
 * group carries the weight w = nsample - rows_of_the_group + 1 of the copies that were dropped:
 *   forward   BN batch statistics weigh that row with w (the max-pool ignores copies anyway);
 *   backward  the row stands for the SUM of the gradients of its w twins: dY = p.G + w (q.Y + t), everything
 *             downstream of dY (ReLU mask, dgrad, wgrad, the scatter-add) is linear in it.
 * Same mathematics as the uncompacted stack (only the summation order of the statistics changes).
 * The number of rows depends on the data: it lives on the device (pcops_rows_t.rows); the M / b*m*s arguments of the
 * *_rows entry points are the UNCOMPACTED row count, i.e. the upper bound the buffers and launches are sized with,
 * and batch-norm divisors (pcops_mlp_bn_finalize / _bn_bwd_coeffs R) stay the uncompacted count.
 * rows == NULL: exactly the entry point without the suffix.  Compacted rows need the wave-stream shapes
 * (>= 8192 rows, channel counts multiples of 8): PCOPS_ERR_UNSUPPORTED otherwise. */
/* TensorFlow-flavoured Adam on flat fp32 buffers of n floats (n % 4 == 0, 16-byte aligned), one launch:
 *   m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  p <- p - lr_t m / (sqrt(v) + epsilon)
 * lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) comes from the caller (tf.train.AdamOptimizer: epsilon outside the
 * bias-corrected root; reference trainers pointnet2/train.py:165-168). */
int pcops_adam_step(long long n, float *p, const float *g, float *m, float *v, float beta1, float beta2, float lr_t,
                    float epsilon, pcops_stream_t stream);
/* The same update, element for element and bit for bit, with lr_t read from DEVICE memory (one float, 4-byte aligned,
 * the same value for every element): the launch then has no argument that changes from step to step, so a training
 * step captured as a HIP graph replays it unchanged while the caller refreshes *lr_t on the same stream ahead of the
 * replay.  Argument checks as pcops_adam_step, and lr_t must not be NULL. */
int pcops_adam_step_dev(long long n, float *p, const float *g, float *m, float *v, float beta1, float beta2,
                        const float *lr_t, float epsilon, pcops_stream_t stream);
/* 1 when every launch of a grouped stack over compacted rows has a kernel for its shape (the *_rows entry points have
 * no tiled fallback): b clouds x m groups x s slots, n source points per cloud, has_q = the first layer has a feature
 * term (its gradient then walks the rows through the inverse index), widths [nlayers] = the layers' output widths
 * (HOST array).  pcops_sa_scatter_rows_supported: the first layer's part of that answer. */
int pcops_gather_stack_rows_supported(int b, int n, int m, int s, int has_q, int nlayers, const int *widths);
int pcops_sa_scatter_rows_supported(int n, int m, int s, int c);
unsigned long long pcops_rows_max_blocks(int b, int m, int s);
/* builds blocks / block_start / rows from pts_cnt (b,m) of pcops_query_ball_point; s % 16 == 0.
 * blocks: 16 * pcops_rows_max_blocks(b,m,s) bytes, block_start: b*m + 1 ints, rows: 1 int. */
int pcops_rows_plan(int b, int m, int s, const int *pts_cnt, void *blocks, int *block_start, int *rows,
                    pcops_stream_t stream);
int pcops_mlp_gemm_fwd_rows(int M, int K, int N, const float *X, int ldx, const float *pro_scale,
                            const float *pro_shift, const float *W, const float *bias, float *Y,
                            float *stats_partial, const float *stat_pivot, const pcops_rows_t *rows,
                            pcops_stream_t stream);
int pcops_mlp_gemm_fwd_xyz_rows(int M, int K, int N, const float *off4, const float *xyzw, const float *pro_scale,
                                const float *pro_shift, const float *W, const float *bias, float *Y,
                                float *stats_partial, const float *stat_pivot, const pcops_rows_t *rows,
                                pcops_stream_t stream);
int pcops_mlp_gemm_dgrad_rows(int M, int K, int Nout, const float *G, const float *Y, const float *p,
                              const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                              int S, const float *pool_scale, const float *pool_shift, const float *Wt,
                              const float *Yprev, const float *prev_scale, const float *prev_shift, float *Gprev,
                              float *stats_partial, const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_mlp_gemm_dgrad_xyz_rows(int M, int K, int Nout, const float *G, const float *Y, const float *p,
                                  const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                                  int S, const float *pool_scale, const float *pool_shift, const float *Wt,
                                  const float *off4, const float *xyzw, const float *prev_scale,
                                  const float *prev_shift, float *Gprev, float *stats_partial, float *xyz_stats,
                                  const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_mlp_wgrad_rows(long long M, int K, int N, const float *X, int ldx, const float *a_scale,
                         const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                         const float *t, const float *gpool, const unsigned char *argmax, int S,
                         const float *pool_scale, const float *pool_shift, float *partial, float *dW, float *db,
                         const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_mlp_wgrad_xyz_rows(long long M, int K, int N, const float *off4, const float *xyzw, const float *a_scale,
                             const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                             const float *t, const float *gpool, const unsigned char *argmax, int S,
                             const float *pool_scale, const float *pool_shift, float *partial, float *dW, float *db,
                             const pcops_rows_t *rows, pcops_stream_t stream);
/* last layer of a max-pooled stack over compacted rows, pooling fused into the epilogue: ypart / ppart
 * [pcops_rows_max_blocks][N] receive, per 16-row block, the selected raw value (max for gamma >= 0, min otherwise)
 * and its row-in-group; pcops_mlp_pool_combine_rows picks per group -> out = relu(scale*ysel + shift), argmax, ysel
 * Y == NULL: the activation is not stored (its backward is the algebraic one, or there is none); the other outputs are
 * bit for bit those of the storing call. */
int pcops_mlp_gemm_fwd_pool_rows_supported(int M, int K, int N);
int pcops_mlp_gemm_fwd_pool_rows(int M, int K, int N, const float *X, int ldx, const float *pro_scale,
                                 const float *pro_shift, const float *W, const float *bias, const float *gamma,
                                 float *Y, float *stats_partial, const float *stat_pivot, float *ypart,
                                 unsigned char *ppart, const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_mlp_pool_combine_rows(long long G, int C, const float *ypart, const unsigned char *ppart,
                                const float *gamma, const float *scale, const float *shift,
                                const pcops_rows_t *rows, float *out, unsigned char *argmax, float *ysel,
                                pcops_stream_t stream);
/* out[g] = max over the rows of group g of relu(scale*Y + shift); argmax = row-in-group of the first maximiser */
int pcops_mlp_bn_relu_maxpool_rows(long long G, int C, const float *Y, const float *scale, const float *shift,
                                   const pcops_rows_t *rows, float *out, unsigned char *argmax, float *ysel,
                                   pcops_stream_t stream);
/* ---- the algebraic backward of a pooled top layer over compacted rows.  With the weight w_r on the first row of a group,
 * dY_r = (p.G)_r + w_r (q.Y_r + t) and sum w_r = M (the uncompacted count); substituting Y = X W + b:
 *   dX_r = w_r (X_r Mq + v) + (p.G)_r W^T                              Mq = W diag(q) W^T, v = W (q.b + t)
 *   dW   = (X^T diag(w) X)(W diag(q)) + (X^T w)(q.b + t)^T + X^T (p.G)
 *   db   = 1^T (p.G) + q.((X^T w) W + M b) + M t
 * The weight enters the dense terms only: the arg-max row of a group is its first maximiser, counted once.
 * pcops_mlp_pool_top_prep / _finish and the small products are the uncompacted ones (finish with M = the uncompacted
 * count).  argmax is the row-in-group in compacted numbering (pcops_mlp_pool_combine_rows); the row of slot (g, a) is
 * 16 block_start[g] + a; rowmap and the addend are indexed by the compacted row (slot = row: addend [M][Kp],
 * addend_rows = M).  The sparse halves are built for MANY SMALL groups (W^T / a group's rows of X held in LDS);
 * pcops_mlp_pool_top_wsparse_rows takes a scratch of pcops_mlp_pool_top_wsparse_rows_partial(Kp, N) floats in front of
 * the row set.  pcops_mlp_gram_rows: gram = X^T diag(w) X, xsum = X^T w (partial as pcops_mlp_gram).
 * pcops_mlp_pool_top_rows_supported is the ONE answer a caller asks for all four (S % 16 == 0, S <= 128, Kp = 64 / 128,
 * N <= 256, the addend within the 32-bit offset of its bounds check).  Sums in a fixed order (deterministic).
 * pcops_mlp_pool_top_addend_rows itself takes any M: the floor on M in that answer belongs to the Gram pass and the dense
 * products. */
int pcops_mlp_pool_top_rows_supported(int M, int Kp, int N, int S);
unsigned long long pcops_mlp_pool_top_wsparse_rows_partial(int Kp, int N);
int pcops_mlp_pool_top_addend_rows(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                                   const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                                   const float *p, const float *Wt, float *addend, int *rowmap, const pcops_rows_t *rows,
                                   pcops_stream_t stream);
int pcops_mlp_gemm_dgrad_top_rows(int M, int Kp, const float *Yprev, const float *prev_scale, const float *prev_shift,
                                  const float *Mq, const float *vconst, const float *addend, long long addend_rows,
                                  const int *rowmap, float *Gprev, float *stats_partial, const pcops_rows_t *rows,
                                  pcops_stream_t stream);
int pcops_mlp_gram_rows(long long M, int Kp, const float *Yprev, int ldx, const float *a_scale, const float *a_shift,
                        float *partial, float *gram, float *xsum, const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_mlp_pool_top_wsparse_rows(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                                    const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                                    const float *p, const float *Yprev, const float *prev_scale, const float *prev_shift,
                                    float *Ssp, float *cfsum, float *partial, const pcops_rows_t *rows,
                                    pcops_stream_t stream);
/* pcops_sa_gather_fwd / pcops_sa_scatter_bwd over compacted rows: Y, off4, G are (rows, c) / (rows, 4) in the
 * compacted order; idx stays the (b,m,s) tensor of the ball query */
int pcops_sa_gather_fwd_rows(int b, int n, int m, int s, int c, const float *Q, const float *Ctr, const float *xyz,
                             const float *new_xyz, const float *Wxyz, const float *bias, const int *idx, float *Y,
                             float *off4, float *stats_partial, const float *stat_pivot, float *moments,
                             const pcops_rows_t *rows, pcops_stream_t stream);
int pcops_sa_scatter_bwd_rows(int b, int n, int m, int s, int c, const float *G, const float *Y, const float *p,
                              const float *q, const float *t, const float *gpool, const unsigned char *argmax,
                              const float *pool_scale, const float *pool_shift, const int *idx, const float *xyz,
                              const float *new_xyz, float *dQ, float *dCtr, float *wpartial, float *dWxyz,
                              float *dbias, const float *fwd_Q, const float *fwd_Ctr, const float *fwd_Wxyz,
                              const float *fwd_bias, void *workspace, const pcops_rows_t *rows,
                              pcops_stream_t stream);

/* ---- the [Q | Ctr] forms of the five entry points above (csrc/edgeconv.hip).  EdgeConv's first conv is linear in the
 * edge feature, concat(x_i, x_j - x_i) W = x_j W_b + x_i (W_a - W_b) (dgcnn/utils/tf_util.py:699-705 + dgcnn.py:39-44):
 * Q = X W_b and Ctr = X (W_a - W_b) + bias are the column halves of ONE product X [W_b | W_a - W_b] with row stride 2 c,
 * and dQ / dCtr the halves of one gradient, so the per-point GEMM, its weight gradient and its data gradient run once
 * instead of twice (and autograd has nothing to add up).  ldq / ldc / lddq / lddc: row strides in floats (multiples of 4,
 * >= c) of Q / Ctr / dQ / dCtr; everything else as in the dense entry points; n == m.  Only shapes
 * pcops_edge_ld_supported() accepts have kernels (64-channel slices, whole 64-group chunks, LDS-resident clouds);
 * PCOPS_ERR_UNSUPPORTED otherwise.  In deterministic mode the QUERY answers 0 (the backward's arg-row sums are LDS float
 * atomics; keep the dense entry points and their ordered kernels); the entry points themselves check the shape only, so a
 * backward whose forward chose this family still runs when the switch is thrown in between.  The sa_* pair is the Q + Ctr form of
 * pcops_sa_gather_fwd / pcops_sa_scatter_bwd (no coordinate term, G materialised, dQ and dCtr both produced). */
int pcops_edge_ld_supported(int b, int n, int m, int s, int c);
int pcops_edge_pool_fwd_ld(int b, int n, int m, int s, int c, const float *Q, int ldq, const float *Ctr, int ldc,
                           const int *idx, const float *gamma, float *SQ, float *qsel, unsigned char *arg,
                           float *stats_partial, const float *stat_pivot, pcops_stream_t stream);
int pcops_edge_pool_out_ld(long long groups, int c, const float *qsel, const float *Ctr, int ldc, const float *scale,
                           const float *shift, float *out, float *ysel, pcops_stream_t stream);
/* ... and a SECOND copy of `out` into a column block of a wider row-major tensor (out2 + g * ld2): DGCNN concatenates the
 * four EdgeConv outputs (dgcnn/models/dgcnn.py:83), so each layer stores its block of the (b, n, 320) tensor on the way
 * out and no concatenation pass (671 MB read + written) runs.  out2 may be NULL (= pcops_edge_pool_out_ld). */
int pcops_edge_pool_out_ld2(long long groups, int c, const float *qsel, const float *Ctr, int ldc, const float *scale,
                            const float *shift, float *out, float *ysel, float *out2, int ld2, pcops_stream_t stream);
int pcops_edge_pool_bwd_ld(int b, int n, int m, int s, int c, const float *Q, int ldq, const float *Ctr, int ldc,
                           const int *idx, const float *gpool, const float *ysel, const float *SQ,
                           const unsigned char *arg, const float *scale, const float *shift, const float *p,
                           const float *q, const float *t, float *dQ, int lddq, float *dCtr, int lddc, void *workspace,
                           pcops_stream_t stream);
int pcops_sa_gather_fwd_ld(int b, int n, int m, int s, int c, const float *Q, int ldq, const float *Ctr, int ldc,
                           const int *idx, float *Y, float *stats_partial, const float *stat_pivot,
                           pcops_stream_t stream);
int pcops_sa_scatter_bwd_ld(int b, int n, int m, int s, int c, const float *G, const float *p, const float *q,
                            const float *t, const int *idx, const float *Q, int ldq, const float *Ctr, int ldc,
                            float *dQ, int lddq, float *dCtr, int lddc, void *workspace, pcops_stream_t stream);

/* the concatenated weight of the [Q | Ctr] form: W1 (2 c, cp) = the reference's EdgeConv kernel [W_a ; W_b] (rows 0..c-1
 * multiply x_i, rows c..2c-1 multiply x_j - x_i), b1 (cp) or NULL -> Wcat (kp, 2 cp) = [W_b | W_a - W_b] (rows c..kp-1
 * zero: the input zero-padded to kp channels), bcat (2 cp) = [0 | b1]; and the backward map dWcat, dbcat -> dW1, db1. */
int pcops_edge_weights_fwd(int c, int cp, int kp, const float *W1, const float *b1, float *Wcat, float *bcat,
                           pcops_stream_t stream);
int pcops_edge_weights_bwd(int c, int cp, const float *dWcat, const float *dbcat, float *dW1, float *db1,
                           pcops_stream_t stream);

/* ------------------------------------------------------------- classifier / T-Net heads (csrc/head.hip)
 * BatchNorm (+ ReLU) of a fully connected layer's output over R rows (the batch) as one launch per direction:
 * fully_connected(..., bn=True) of pointnet2/utils/tf_util.py:327-363 (batch_norm_for_fc :534-546) and
 * dgcnn/utils/tf_util.py:317-354 (batch_norm_template :462-499).  x, y, dy, dx (R, C) dense.
 *   training != 0: batch mean and BIASED variance normalise; moving_mean / moving_var are updated in place,
 *                  m <- decay m + (1 - decay) batch, the variance fed being var R / (R - 1) when unbiased_moving_var
 *                  (the pointnet2 flavour) and var otherwise (the DGCNN flavour);
 *   training == 0: the moving statistics normalise and nothing is updated.
 * save_mean / save_rstd (C) receive the statistics used (the backward's inputs).  relu != 0: y = max(., 0) and the
 * backward masks dy with y > 0.  Backward: dgamma = sum g xhat, dbeta = sum g, dx = gamma rstd (g - dbeta / R - xhat
 * dgamma / R), or gamma rstd g through frozen statistics (training == 0). */
int pcops_fc_bn_fwd(int R, int C, const float *x, const float *gamma, const float *beta, float *moving_mean,
                    float *moving_var, int training, float decay, float eps, int unbiased_moving_var, int relu,
                    float *y, float *save_mean, float *save_rstd, pcops_stream_t stream);
int pcops_fc_bn_bwd(int R, int C, const float *dy, const float *x, const float *y, const float *gamma,
                    const float *save_mean, const float *save_rstd, int training, int relu, float *dx,
                    float *dgamma, float *dbeta, pcops_stream_t stream);

/* The classification loss of a batch and its gradient in one launch: mean softmax cross entropy against
 * q = s / C + (1 - s) onehot(labels) -- tf.losses.softmax_cross_entropy(..., label_smoothing = s) of dgcnn/models/dgcnn.py:99-105;
 * s = 0 is the sparse softmax cross entropy + reduce_mean of pointnet2/models/pointnet2_cls_ssg.py:47-53 and, over b n rows of
 * two classes, the per-point mask loss of pointnet2_cls_bga.py:94-98 (equal point counts: the mean of the clouds' means is the
 * mean of all rows).  dlogits [R][C] = (softmax - q) / R (the gradient for an upstream factor of 1; the caller scales).
 * loss [pcops_softmax_ce_blocks(R)]: one workgroup up to 4096 rows -- loss[0] is the loss --, several beyond, each leaving
 * its rows' share of the mean (the caller adds them up).  Fixed summation order. */
int pcops_softmax_ce_blocks(int R);
int pcops_softmax_ce(int R, int C, const float *logits, const int *labels, float label_smoothing, float *loss,
                     float *dlogits, pcops_stream_t stream);
/* The interpolation weights of pointnet_fp_module (pointnet_util.py:212-215) from three_nn's squared distances:
 * weight (b, n, 3) = inv / sum(inv), inv = 1 / max(dist, 1e-10); dist = +inf (fewer than three known points) -> 0. */
int pcops_three_nn_weights(int b, int n, const float *dist, float *weight, pcops_stream_t stream);

/* the learned 3 x 3 input transform applied to a cloud (tf.matmul(point_cloud, transform): dgcnn/models/dgcnn.py:37,
 * pointnet/models/pointnet_cls.py:27): out (b, n, 3) = x (b, n, 3) T (b, 3, 3); backward dT (b, 3, 3) = x^T grad_out per cloud in a
 * fixed order, dx = grad_out T^T (dx may be NULL: the input cloud needs no gradient). */
int pcops_transform3_fwd(int b, int n, const float *x, const float *T, float *out, pcops_stream_t stream);
int pcops_transform3_bwd(int b, int n, const float *x, const float *T, const float *grad_out, float *dT, float *dx,
                         pcops_stream_t stream);

/* ------------------------------------------------------------------ SpiderConv (csrc/spider.hip)
 * One SpiderConv layer of SpiderCNN (SpiderCNN/utils/tf_util.py:127-236, group_norm_for_conv :407-429).  P = b n centre
 * points, k neighbours, t = 5 Taylor channels, feat (b, n, c), idx (b, n, k) int32 in [0, n) (self first), delta (b, n, k, 3)
 * = neighbour - centre.  theta (19, t) holds the weight_* variables in the order x y z xyz xy yz xz xx yy zz xxy xyy xxz
 * xzz yyz yzz xxx yyy zzz, tbias (t) is taylor/biases:
 *   g (b, n, k, t)        g[p,j,t] = tbias[t] + sum_m theta[m,t] phi_m(delta[p,j])
 *   y (b, n, o)           y[p,o] = bias[o] + sum_{j,c,t} feat[idx[p,j],c] g[p,j,t] w[(j c_ + c) t_ + t][o]; w is conv/weights
 *                         [1, k, c t, o] read as a (k c t) x o row-major matrix.  The expanded operand A[p,(j,c,t)] is formed
 *                         tile by tile in LDS and never written to memory (fp32 MFMA).
 * Backward: wgrad dw = A^T dy, dbias = column sums of dy (may be NULL); dgrad dfeat_grouped (b, n, k, c) = sum_t (dy w^T) g
 * (NULL: not wanted, e.g. the raw cloud of the first layer) and dg (b, n, k, t) = sum_c (dy w^T) feat[idx]; the caller
 * scatters dfeat_grouped with pcops_group_point_grad / pcops_scatter_rows_sorted; taylor_bwd reduces dg to dtheta (19, t)
 * and dtbias (t).  Every output is written whole (no accumulation); every sum is taken in a fixed order, with no float
 * atomics, so two backward passes are bit-identical whatever pcops_set_deterministic says.
 * Supported: 1 <= k <= 64 and k <= n (PCOPS_ERR_BAD_ARGUMENT), t == 5, 1 <= c <= 256, o % 16 == 0 with 16 <= o <= 512,
 * b n k max(c, t) < 2^31; PCOPS_ERR_UNSUPPORTED outside.  Workspaces are caller-owned device buffers of the queried size
 * (0: may be NULL). */
int pcops_spider_taylor_fwd(long long rows, int t, const float *delta, const float *theta, const float *tbias, float *g,
                            pcops_stream_t stream);
unsigned long long pcops_spider_taylor_bwd_workspace_bytes(long long rows, int t);
int pcops_spider_taylor_bwd(long long rows, int t, const float *delta, const float *dg, float *dtheta, float *dtbias,
                            void *workspace, pcops_stream_t stream);
int pcops_spider_conv_fwd(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx, const float *g,
                          const float *w, const float *bias, float *y, pcops_stream_t stream);
unsigned long long pcops_spider_conv_wgrad_workspace_bytes(int b, int n, int c, int k, int t, int o);
int pcops_spider_conv_wgrad(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx, const float *g,
                            const float *dy, float *dw, float *dbias, void *workspace, pcops_stream_t stream);
int pcops_spider_conv_dgrad(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx, const float *g,
                            const float *w, const float *dy, float *dfeat_grouped, float *dg, pcops_stream_t stream);

/* Group norm + ReLU over x (b, n, c): `groups` groups of c / groups contiguous channels, each normalised per cloud over
 * its n points and channels with the biased variance (two-pass moments), then y = max(gamma xhat + beta, 0).  mean / rstd
 * (b, groups) receive the statistics.  Backward through the ReLU mask y > 0: dx, and dgamma / dbeta summed over the
 * clouds in ascending order through pcops_group_norm_relu_workspace_bytes(b, c) bytes of workspace.
 * groups must divide c (PCOPS_ERR_BAD_ARGUMENT); c / groups <= 256 and c <= 4096 (PCOPS_ERR_UNSUPPORTED). */
unsigned long long pcops_group_norm_relu_workspace_bytes(int b, int c);
int pcops_group_norm_relu_fwd(int b, int n, int c, int groups, float eps, const float *x, const float *gamma,
                              const float *beta, float *y, float *mean, float *rstd, pcops_stream_t stream);
int pcops_group_norm_relu_bwd(int b, int n, int c, int groups, const float *dout, const float *x, const float *y,
                              const float *gamma, const float *mean, const float *rstd, float *dx, float *dgamma,
                              float *dbeta, void *workspace, pcops_stream_t stream);

/* ------------------------------------------------------------------ 3DmFV-Net (csrc/mfv.hip)
 * The 3DmFV representation (3DmFV-Net/utils/tf_util.py:578-652, get_3dmfv): points (b, n, 3) against a fixed mixture of k
 * diagonal Gaussians w (k), mu (k, 3), sigma (k, 3) -- sigma is the STANDARD DEVIATION.  Per (point, Gaussian)
 * Q = w N(x) / sum_k w N(x), z = (x - mu) / sigma; per Gaussian over the points max, sum of Q - w and max, min, sum per
 * axis of Q z and of Q (z^2 - 1); scaled by 1 / (n sqrt(w)) resp. 1 / (n sqrt(2 w)), power-normalised sign(x) sqrt|x| and
 * L2-normalised over the Gaussians per (cloud, row) as x / sqrt(max(sum x^2, 1e-12)).  fv (b, 20, k) in the reference's row
 * order: d_pi max, sum; d_mu max xyz, min xyz, sum xyz; d_sigma max xyz, min xyz, sum xyz.  voxel_major != 0 writes
 * (k, b, 20) instead: the voxel-major activation the convolutions below take (Gaussian index = voxel index).
 * Nothing of n k elements is written to memory; chunk partials (512 points) go to pcops_fv3d_workspace_bytes(b, n, k) bytes
 * of caller-owned workspace and are folded in ascending chunk order: no float atomics, bit-identical run to run.
 * Supported: n >= 1, 1 <= k <= 512, b <= 65535, b n 3 < 2^31; PCOPS_ERR_UNSUPPORTED outside, before any launch. */
unsigned long long pcops_fv3d_workspace_bytes(int b, int n, int k);
int pcops_fv3d_fwd(int b, int n, int k, int voxel_major, const float *points, const float *w, const float *mu,
                   const float *sigma, float *fv, void *workspace, pcops_stream_t stream);

/* 3-D convolution with k^3 taps, k in {3, 5}, stride 1, SAME padding, on a cubic grid of r^3 voxels (r <= 8).  Activations
 * are VOXEL-MAJOR: x (r^3, b, cin), y (r^3, b, cout), voxel index (i r + j) r + l; w (k, k, k, cin, cout) as in the reference
 * (tf_util.py:290), bias (cout) or NULL.  y[v] = bias + sum over the taps t with v + t inside the grid of x[v + t] w[t]: one
 * dense fp32 MFMA product per in-grid tap; no expanded operand exists and no matrix instruction is spent on padding.
 * dgrad: dx (r^3, b, cin) through the forward kernel on the mirrored, transposed weights, which one small launch writes
 * into pcops_conv3d_dgrad_workspace_bytes bytes of workspace.  wgrad: dw (k, k, k, cin, cout), dbias (cout) or NULL; the rows
 * of a tap are split pcops_conv3d_wgrad_splits ways (1, 2, 4, 8 or 16) and the partials added in ascending order through
 * pcops_conv3d_wgrad_workspace_bytes bytes (0 with one split: direct store, workspace may be NULL).  Every output is written
 * whole; no float atomics.  Supported: cin, cout multiples of 16 up to 512, r^3 b max(cin, cout) < 2^31;
 * PCOPS_ERR_UNSUPPORTED outside, before any launch. */
int pcops_conv3d_fwd(int b, int r, int k, int cin, int cout, const float *x, const float *w, const float *bias, float *y,
                     pcops_stream_t stream);
unsigned long long pcops_conv3d_dgrad_workspace_bytes(int b, int r, int k, int cin, int cout);
int pcops_conv3d_dgrad(int b, int r, int k, int cin, int cout, const float *w, const float *dy, float *dx, void *workspace,
                       pcops_stream_t stream);
int pcops_conv3d_wgrad_splits(int b, int r, int k, int cin, int cout);
unsigned long long pcops_conv3d_wgrad_workspace_bytes(int b, int r, int k, int cin, int cout);
int pcops_conv3d_wgrad(int b, int r, int k, int cin, int cout, const float *x, const float *dy, float *dw, float *dbias,
                       void *workspace, pcops_stream_t stream);

/* ------------------------------------------------------------------ X-Conv contraction of PointCNN (csrc/xconv.hip)
 * The gather, the concat, the product with the X-transform and the depthwise (1, K) half of the separable convolution of
 * one X-Conv layer (PointCNN/pointcnn.py:28-44) in one launch.  b clouds of n points, p representative points per cloud,
 * k neighbours each, c = c1 + c2 channels, depth multiplier dm:
 *   lifted (b, p, k, c1)   the features lifted from the local coordinates (nn_fts_from_pts)
 *   fts    (b, n, c2)      the previous layer's features, idx (b, p, k) int32 in [0, n) per cloud; both NULL with c2 == 0
 *                          (the first layer)
 *   X      (b, p, k, k)    the X-transform, row k' column k
 *   wd     (k, c, dm)      the depthwise kernel [1, k, c, dm] of fts_conv
 *   Fin[q,j,:] = concat(lifted[q,j,:], fts[idx[q,j],:])
 *   out (b, p, c dm)       out[q, ch dm + m] = sum_k' wd[k',ch,m] sum_j X[q,k',j] Fin[q,j,ch]     (TF's channel order)
 * Neither Fin nor X Fin is written to memory: one wave forms the 16 x 16 tile of a point and 16 channels with fp32 MFMA
 * (k zero-padded to 16) and contracts it over k' in registers.
 * dgrad: dX (b, p, k, k), dlifted (b, p, k, c1) and dfts_grouped (b, p, k, c2) -- the gradient of the GATHERED rows, NULL
 * when not wanted or c2 == 0; the caller scatters it with pcops_group_point_grad / pcops_scatter_rows_sorted.
 * wgrad: dwd (k, c, dm), X Fin recomputed.  The b p points are cut into pcops_xconv_wgrad_splits contiguous ranges (a power
 * of two up to 64, whole 16-point steps, at least 16 points each); with more than one, the partial sums go to
 * pcops_xconv_wgrad_workspace_bytes bytes of caller-owned workspace (0 with one split: direct store, workspace may be NULL)
 * and are added in ascending order.  Every output is written whole; every sum is taken in a fixed order with no float
 * atomics, so two calls give the same bits whatever pcops_set_deterministic says.
 * Channel groups: a wave walks the 16-channel tiles of its point one after the other, so a wide layer (the X-DeConv layers of
 * pointcnn_seg: up to 576 channels on 4096 points) is a long dependent chain on few waves.  With tiles = ceil(c / 16) > 16
 * and PCOPS_OPT_XCONV_CHANNEL_GROUPS on, fwd and dgrad_ws launch pcops_xconv_channel_groups = ceil(tiles / 8) workgroups per
 * 16 points, group g owning the tiles [g t, (g + 1) t), t = ceil(tiles / groups) (no group is empty, none holds more than 8),
 * and staging only its own columns of wd.  Channels never mix in out, dlifted and dfts_grouped: the same bits as with one group.
 * dX sums over the channels: with more than one group, group g writes its (b p, k, k) partial sum to slice g of
 * pcops_xconv_dgrad_workspace_bytes = groups b p k k 4 bytes of caller-owned workspace and one pass adds the slices in
 * ascending order (0 bytes and workspace NULL with one group, where dgrad_ws launches what dgrad launches).  pcops_xconv_dgrad
 * itself always runs one group.  c <= 256 is one group whatever the option says; the query answers 0 for a shape the
 * launchers refuse and for b == 0.
 * Supported (pcops_xconv_supported): 1 <= k <= 16, c1 >= 1, c2 >= 0, 1 <= dm <= 4, c dm <= 960 (16 rows of wd in LDS);
 * b p k max(c dm, k) < 2^31 and b n c2 < 2^31.  PCOPS_ERR_UNSUPPORTED outside, before any launch and any pointer check. */
int pcops_xconv_supported(int k, int c1, int c2, int dm);
int pcops_xconv_channel_groups(int b, int n, int p, int k, int c1, int c2, int dm);
unsigned long long pcops_xconv_dgrad_workspace_bytes(int b, int n, int p, int k, int c1, int c2, int dm);
int pcops_xconv_dgrad_ws(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                         const int *idx, const float *X, const float *wd, const float *dout, float *dX, float *dlifted,
                         float *dfts_grouped, void *workspace, pcops_stream_t stream);
int pcops_xconv_fwd(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                    const int *idx, const float *X, const float *wd, float *out, pcops_stream_t stream);
int pcops_xconv_dgrad(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                      const int *idx, const float *X, const float *wd, const float *dout, float *dX, float *dlifted,
                      float *dfts_grouped, pcops_stream_t stream);
int pcops_xconv_wgrad_splits(int b, int n, int p, int k, int c1, int c2, int dm);
unsigned long long pcops_xconv_wgrad_workspace_bytes(int b, int n, int p, int k, int c1, int c2, int dm);
int pcops_xconv_wgrad(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                      const int *idx, const float *X, const float *dout, float *dwd, void *workspace,
                      pcops_stream_t stream);

/* ------------------------------------------------------------------ PointNet's per-cloud feature transform (csrc/tnet.hip)
 * tf.matmul(net, transform) of pointnet/models/pointnet_cls.py:47 with a DIFFERENT k x k matrix per cloud, and the
 * orthogonality regulariser of :86-91.  k is the transform's width; only k == 64 is built.
 *   X, out, G, dX (b, n, k) row-major;  T, dT (b, k, k);  every pointer, the workspace included, 16-byte aligned
 *   fwd:  out[c][p][:] = X[c][p][:] T[c]
 *   bwd:  dX[c] = G[c] T[c]^T (dX may be NULL: not wanted),  dT[c] = X[c]^T G[c], one pass over G.  A cloud's points are cut
 *         into pcops_transformk_bwd_splits contiguous ranges: the largest power of two <= min(ceil(512 / b), ceil(n / 64), 16),
 *         each range ceil(ceil(n / splits) / 64) 64 points (trailing ranges may hold no point and contribute zeros).  One
 *         split stores dT directly (workspace may be NULL); more write partial sums to pcops_transformk_workspace_bytes =
 *         b splits k k 4 bytes of caller-owned workspace and a second kernel adds them in ascending order.
 *   ortho: Gm = T[c] T[c]^T - I, loss_parts[c] = weight / 2 sum Gm^2, dT[c] = 2 weight Gm T[c] -- loss and gradient from one
 *         launch, one workgroup per cloud.  The loss of tf.nn.l2_loss is the SUM of loss_parts over the clouds (the caller's).
 * fp32 operands on the fp32 matrix pipe, no split operands; every sum in a fixed order, no float atomics: two calls give the
 * same bits whatever pcops_set_deterministic says.
 * Supported (pcops_transformk_supported): k == 64, 1 <= b <= 65535, n >= 1, b n k < 2^31; pcops_ortho_reg: k == 64,
 * 1 <= b <= 65535.  PCOPS_ERR_UNSUPPORTED outside, before any launch and any pointer check; the queries answer 0. */
int pcops_transformk_supported(int b, int n, int k);
int pcops_transformk_bwd_splits(int b, int n, int k);
unsigned long long pcops_transformk_workspace_bytes(int b, int n, int k);
int pcops_transformk_fwd(int b, int n, int k, const float *X, const float *T, float *out, pcops_stream_t stream);
int pcops_transformk_bwd(int b, int n, int k, const float *X, const float *T, const float *G, float *dX, float *dT,
                         void *workspace, pcops_stream_t stream);
int pcops_ortho_reg(int b, int k, const float *T, float weight, float *loss_parts, float *dT, pcops_stream_t stream);

/* ---------------------------------------------- first conv of PointNet's segmentation heads (csrc/cloudpoint.hip)
 * conv6 of pointnet/models/pointnet_seg.py:81-88 and pointnet_partseg.py:66-73 on concat([point_feat (64) | tiled global feature
 * (1024)]): the per-cloud columns are one row Ctr[cloud] = global W_c + bias per cloud (the caller's small product), the
 * per-point columns a k = 64 deep product that is evaluated INSIDE the streaming pass -- neither Q = X Wx nor its gradient
 * dQ ever exists in memory (the pcops_cloud_bias_* form of the same layer reads and writes both).
 *   X, dX (b n, k);  Wx, dWx (k, c);  Ctr, dCtr (b, c);  Y, G (b n, c), all row-major; every pointer, the workspace included,
 *   16-byte aligned;  p, q, t [c]: the coefficients of pcops_mlp_bn_bwd_coeffs
 *   fwd:  Y[r, :] = X[r, :] Wx + Ctr[r / n, :].  stats_partial (NULL: evaluation mode, no statistics):
 *         [pcops_cloud_point_rows(b, n) = b ceil(n / 128)][2][c] sums of (y - pivot) and (y - pivot)^2 over the rows of one
 *         workgroup -- the layout pcops_cloud_bias_fwd produces and pcops_mlp_bn_finalize consumes; stat_pivot [c] (NULL: 0).
 *         A workgroup holds 128 points of ONE cloud; the tail tile of a cloud is masked.
 *   bwd:  D = p G + q Y + t per element, never stored;  dX = D Wx^T (dX may be NULL: not wanted),  dWx = X^T D,
 *         dCtr[cloud] = the sum of D over the cloud's rows.  A cloud's points are cut into s contiguous ranges, s = the largest
 *         power of two <= min(ceil(512 / b), ceil(n / 64), 16), each ceil(ceil(n / s) / 64) 64 points (trailing ranges may hold
 *         no point and contribute zeros); pcops_cloud_point_bwd_parts = b s is the number of partial dWx matrices.  One part
 *         stores dWx and dCtr directly (workspace may be NULL); more write partial sums to pcops_cloud_point_bwd_ws bytes of
 *         caller-owned workspace ([parts][k][c], then [parts][c] where s > 1) and one launch each adds them in ascending order.
 *         Layers wider than 512 channels run the pass once per 512 channels; the later passes add to the first's dX.
 * fp32 operands on the fp32 matrix pipe, no split operands; every sum in a fixed order, no float atomics: two calls give the
 * same bits whatever pcops_set_deterministic says.
 * Supported (pcops_cloud_point_supported): k == 64, c % 64 == 0, 64 <= c <= 1024, 1 <= b <= 65535, n >= 1, b n c < 2^31.
 * PCOPS_ERR_UNSUPPORTED outside, before any launch and any pointer check; the queries answer 0. */
int pcops_cloud_point_supported(int b, int n, int k, int c);
int pcops_cloud_point_rows(int b, int n);
int pcops_cloud_point_fwd(int b, int n, int k, int c, const float *X, const float *Wx, const float *Ctr, float *Y,
                          float *stats_partial, const float *stat_pivot, pcops_stream_t stream);
int pcops_cloud_point_bwd_parts(int b, int n, int c);
unsigned long long pcops_cloud_point_bwd_ws(int b, int n, int k, int c);
int pcops_cloud_point_bwd(int b, int n, int k, int c, const float *G, const float *Y, const float *p, const float *q,
                          const float *t, const float *X, const float *Wx, float *dX, float *dWx, float *dCtr, void *workspace,
                          pcops_stream_t stream);

/* ---- Device-resident feed (feed.hip): one launch builds a training step's batch from a set that
 * lives on the device -- it picks the clouds and their points, gathers labels and the per-point mask / parts, and applies the
 * augmentation recipe with counter-based random numbers, so the launch replays unchanged inside a captured step.
 *   set:    pts (P, 3) all clouds one after the other; offsets (K + 1) first point of every cloud, or NULL: a dense set of
 *           ntot points per cloud (ntot is not read for a ragged set); labels (K); side: one value per point of pts (mask or
 *           parts), or NULL.
 *   epoch:  order (K) the epoch's cloud order, values in [0, K).  mode 0: output point j reads source point idx_pts[j]
 *           (n values in [0, ntot), one list shared by every cloud; dense sets only).  mode 1: output point j reads source
 *           point perm(j) of the cloud's own pseudo-random permutation (below; idx_pts is not read).
 *   step:   params = four ints in DEVICE memory {first, step, epoch, 0}, read by the kernel (pcops_feed_set_params writes
 *           them with an ordinary kernel whose values are launch arguments); seed, the recipe and its constants by value.
 *   out:    x (B, n, 3), y (B), m (B, n) or NULL (with side == NULL neither is touched).
 * Row r is cloud c = order[first + r].  A row with first + r >= K (or first + r < 0) is written as zeros with label -1, and
 * nothing of the set is read for it.  An order / idx_pts entry outside its range is outside the contract; the kernel still
 * reads nothing outside the set for it (the row, or the point, is written as zeros).
 * min_points: the smallest cloud of the set, known to the host (ntot for a dense set): n > min_points is PCOPS_ERR_BAD_SHAPE.
 * K, n <= 0, B < 0, ntot <= 0 for a dense set: PCOPS_ERR_BAD_SHAPE; mode / recipe outside their values, mode 0 on a ragged
 * set, clip <= 0 or smin > smax with a recipe that reads them: PCOPS_ERR_BAD_ARGUMENT; B > 65535: PCOPS_ERR_UNSUPPORTED;
 * B == 0: PCOPS_OK, nothing launched.  Nothing is written when a status other than PCOPS_OK comes back.
 *
 * Recipes (every product and sum a separate fp32 operation, in this order):
 *   0  the gather only.
 *   1  rotation about Y by theta = 2 pi u(w0) of the cloud's draw, x' = x c - z s, z' = x s + z c (provider.rotate_point_cloud's
 *      row-vector convention), then the jitter.
 *   2  per-axis scale s_k = smin + (smax - smin) u(w_k) of the cloud's draw, then per-axis translation
 *      t_k = (2 u(w_k) - 1) tval of the cloud's second draw: v_k s_k + t_k; then the jitter (mfv3d_net_cls.augment).
 *   jitter: v_k + min(max(sigma z_k, -clip), clip) with the point's normals z_0, z_1, z_2.
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53 on word 0 and 0xCD9E8D57 on word 2, key increments 0x9E3779B9 and
 * 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32).  Counters, g = first + r being the GLOBAL position of the cloud in the
 * epoch's order (a batch does not depend on how it is split over ranks):
 *   the cloud's draws (g, step, 0, TAG_CLOUD) and (g, step, 1, TAG_CLOUD); the normals of output point j (g, step, j, TAG_JIT);
 *   the permutation keys of cloud c (c, epoch, t, TAG_PERM), t = 0, 1 (key[0..3], key[4..7]).
 * u(w) = ((w >> 9) + 0.5) 2^-23, exact in fp32 and never 0 or 1.  Normals by Box-Muller: z0 = sqrt(-2 ln u(w0)) cos(2 pi u(w1)),
 * z1 = sqrt(-2 ln u(w0)) sin(2 pi u(w1)), z2 = sqrt(-2 ln u(w2)) cos(2 pi u(w3)).
 * Permutation of a cloud of n_i points: an 8-round unbalanced Feistel network over bits = max(bit_length(n_i - 1), 2) bits
 * with cycle walking.  a = bits / 2, b = bits - a, L = x >> b, R = x & (2^b - 1), (wl, wr) = (a, b); for r = 0..7:
 * (L, R) <- (R, L ^ F(R, key[r], wl)), swap wl and wr; x' = (L << b) | R, repeated while x' >= n_i.
 * F(v, k, w) in 32-bit arithmetic: v ^= k; v *= 0x9E3779B1; v ^= v >> 15; v *= 0x85EBCA6B; v ^= v >> 13; v & (2^w - 1). */
#define PCOPS_FEED_TAG_CLOUD 0x434c4f55u   /* "CLOU" */
#define PCOPS_FEED_TAG_JIT   0x4a495454u   /* "JITT" */
#define PCOPS_FEED_TAG_PERM  0x5045524du   /* "PERM" */
int pcops_feed_set_params(int first, int step, int epoch, int *params, pcops_stream_t stream);
int pcops_feed_batch(int K, long long ntot, int B, int n, int mode, int recipe, long long min_points, const float *pts,
                     const long long *offsets, const long long *labels, const long long *side, const int *order,
                     const int *idx_pts, const int *params, unsigned long long seed, float sigma, float clip, float smin,
                     float smax, float tval, float *x, long long *y, long long *m, pcops_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCOPS_H */
