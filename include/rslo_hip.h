/*
 * rslo_hip.h -- C ABI of librslo_hip.so, the MI355X (gfx950) implementation of the
 * RSLO two-frame LiDAR-odometry hot path.
 *
 * Boundary rules
 *   - extern "C", plain device pointers + sizes, no torch types.  Every pointer is a
 *     DEVICE pointer unless the parameter name starts with h_.
 *   - The caller owns every buffer (inputs, outputs, workspaces).  Nothing is allocated
 *     or freed inside the library; *_ws_bytes() functions size the workspaces.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises.  Data-dependent counts are written to device ints the caller reads.
 *   - Return value: 0 on success, a negative RSLO_E* code otherwise; rslo_last_error()
 *     gives the text (thread-local).
 *   - Coordinates are int32 (b, z, y, x); features are row-major fp32 [rows, channels];
 *     sparse-conv weights are [K = kz*ky*kx, Cin, Cout] (a view of spconv's
 *     [kz,ky,kx,Cin,Cout]); a neighbour table nbr[rows*K] holds the contributing row of
 *     the other side for kernel offset k, or -1.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * DecaYale/RSLO tree).  The spconv_plus / apex / kornia sources are not part of that tree
 * (Dockerfile:55-61,93-97; freeze.yml:212); for those the call site is cited.
 */
#ifndef RSLO_HIP_H_
#define RSLO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RSLO_API __attribute__((visibility("default")))
#else
#define RSLO_API
#endif

#define RSLO_OK 0
#define RSLO_EINVAL (-1)   /* bad argument / unsupported shape                         */
#define RSLO_ELAUNCH (-2)  /* hipLaunch / runtime error                                */
#define RSLO_ERANGE (-3)   /* linear voxel index does not fit the 32-bit key space     */
#define RSLO_EWS (-4)      /* workspace too small                                      */

RSLO_API int rslo_abi_version(void);
RSLO_API const char *rslo_last_error(void);

/* ------------------------------------------------------------------------------------
 * a1  Voxelization.  Replaces spconv.utils.VoxelGenerator.generate
 *     (rslo/builder/voxel_builder.py:36-54,83-94; called rslo/data/preprocess.py:493).
 * points [P,F] fp32 (x,y,z first).  First-come voxel numbering in point order, at most
 * T points per voxel kept in point order, processing stops at the first point that would
 * open voxel number max_voxels, coordinates stored (z,y,x).
 * Outputs are sized for max_voxels; rows >= *d_nvox are zero.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_voxelize_ws_bytes(int64_t P);
RSLO_API int rslo_voxelize(const float *points, int64_t P, int F, const float *h_range6,
                  const float *h_vsize3, const int32_t *h_grid_xyz, int T, int max_voxels,
                  void *ws, size_t ws_bytes, float *voxels /*[max_voxels,T,F]*/,
                  int32_t *coords /*[max_voxels,3] zyx*/, int32_t *num_points /*[max_voxels]*/,
                  int32_t *d_nvox /*[1]*/, void *stream);

/* a4  SimpleVoxel_XYZINormalC.forward (rslo/models/voxel_encoder.py:258-280):
 *     per-voxel mean of the F features, channels 4:7 divided by (norm + 1e-12). */
RSLO_API int rslo_vfe_mean(const float *voxels /*[M,T,F]*/, const int32_t *num_points /*[M]*/, int64_t M,
                  int T, int F, float *out /*[M,F]*/, void *stream);

/* ------------------------------------------------------------------------------------
 * a5  Site index + rulebooks.  Replace the implicit indice-pair builds behind
 *     spconv.SparseConvTensor / SubMConv3d / SparseConv3d / SparseInverseConv3d
 *     (rslo/models/middle.py:119-213,223-225).
 * The site index is an open-addressing hash: keys[cap] (uint32 linear index, 0xFFFFFFFF =
 * empty), vals[cap] (row).  cap = rslo_hash_capacity(n) (power of two >= 2n).
 * ------------------------------------------------------------------------------------ */
RSLO_API int64_t rslo_hash_capacity(int64_t n);
RSLO_API int rslo_hash_build(const int32_t *coords /*[N,4]*/, int64_t N, int B, const int32_t *h_dims3,
                    uint32_t *keys, int32_t *vals, int64_t cap, void *stream);
/* SubM: output set == input set in the given order; nbr[o][k] = row at coords[o]+(k-ks/2). */
RSLO_API int rslo_rulebook_subm(const int32_t *coords, int64_t N, int B, const int32_t *h_dims3,
                       const int32_t *h_ks3, const uint32_t *keys, const int32_t *vals, int64_t cap,
                       int32_t *nbr /*[N,K]*/, void *stream);
/* Strided conv, step 1: mark the output sites (in = out*stride - pad + k) in a bitmap over
 * the output volume and rank them; *d_count receives the number of output sites M.
 * words = rslo_conv_bitmap_words(B, out_dims).  scan_ws: rslo_scan_ws_bytes(words). */
RSLO_API int64_t rslo_conv_bitmap_words(int B, const int32_t *h_out_dims3);
RSLO_API size_t rslo_scan_ws_bytes(int64_t n);
RSLO_API int rslo_conv_out_count(const int32_t *coords_in, int64_t N, int B, const int32_t *h_ks3,
                        const int32_t *h_stride3, const int32_t *h_pad3, const int32_t *h_out_dims3,
                        uint32_t *bitmap /*[words]*/, int32_t *word_prefix /*[words]*/, int64_t words,
                        void *scan_ws, size_t scan_ws_bytes, int32_t *d_count /*[1]*/, void *stream);
/* step 2: emit the M output coordinates in ascending linear-index order. */
RSLO_API int rslo_conv_out_coords(const uint32_t *bitmap, const int32_t *word_prefix, int64_t words, int B,
                         const int32_t *h_out_dims3, int32_t *out_coords /*[M,4]*/, int64_t M,
                         void *stream);
/* step 3: nbr[o][k] = input row at out*stride - pad + k (probe of the INPUT site index). */
RSLO_API int rslo_rulebook_conv(const int32_t *coords_out, int64_t M, int B, const int32_t *h_in_dims3,
                       const int32_t *h_ks3, const int32_t *h_stride3, const int32_t *h_pad3,
                       const uint32_t *in_keys, const int32_t *in_vals, int64_t in_cap,
                       int32_t *nbr /*[M,K]*/, void *stream);
/* step 4: nbrT[i][k] = output row o with o*stride - pad + k == in (probe of the OUTPUT index);
 * the table the dgrad and SparseInverseConv3d use. */
RSLO_API int rslo_rulebook_conv_T(const int32_t *coords_in, int64_t N, int B, const int32_t *h_out_dims3,
                         const int32_t *h_ks3, const int32_t *h_stride3, const int32_t *h_pad3,
                         const uint32_t *out_keys, const int32_t *out_vals, int64_t out_cap,
                         int32_t *nbrT /*[N,K]*/, void *stream);

/* ------------------------------------------------------------------------------------
 * a6/a7  Sparse convolution arithmetic (spconv SubMConv3d / SparseConv3d /
 *        SparseInverseConv3d forward + backward; call sites middle.py:119-213).
 * fwd : out[o] = act( bias + sum_k in[nbr[o][k]] . W[kk] ),  kk = flip_k ? K-1-k : k
 *       act = LeakyReLU(slope) fused when slope != 1 (middle.py:99-101,123...).
 * dgrad: din[i] = sum_k dout[nbrT[i][k]] . W[kk]^T   (for SubM pass nbr and flip_k=1)
 * wgrad: dW[k]  = sum_o in[nbr[o][k]]^T dout[o]      (deterministic two-stage reduce)
 * Supported channel counts: 1..64 on both sides.
 * ------------------------------------------------------------------------------------ */
/*     row_order (int32 [n_out] or NULL): the order in which the table rows are grouped into the kernels' 16/32-row tiles
 *     (rslo_rulebook_row_order).  Purely a scheduling hint: out[o] is written for every o and does not depend on it.
 *     n_live_dev (device int32 word or NULL = all rows; rslo_spconv_fwd and rslo_spconv_fwd_split).  Round 6, the replayed
 *     inference pass (evaluate.py:363-408 -> rslo/models/middle.py:219-245 per frame; rslo_amd/inference.py): a
 *     capacity-laid-out rulebook has more rows than the scan has sites, the rows past the level's count being padding rows
 *     (rslo_plan_encoder_pad_tails), and the count lives in a device word.  Workgroups whose rows all lie at or past
 *     *n_live_dev return at once -- their output rows are left unwritten; nothing reads a padding row.  Ignored with a row
 *     order. */
RSLO_API int rslo_spconv_fwd(const float *in, int cin, const float *W, const float *bias, const int32_t *nbr,
                    const int32_t *row_order, int64_t n_out, int K, int cout, int flip_k, float act_slope,
                    float *out, const int32_t *n_live_dev, void *stream);
RSLO_API int rslo_spconv_dgrad(const float *dout, int cout, const float *W, const int32_t *nbrT,
                      const int32_t *row_order, int64_t n_in, int K, int cin, int flip_k, float *din, void *stream);
/*     W [K,Cin,Cout] -> Wt [K,Cout,Cin].  rslo_spconv_fwd(dout, Cout, Wt, NULL, nbrT, ...) then equals
 *     rslo_spconv_dgrad(dout, Cout, W, nbrT, ...) with weight reads contiguous along the lane index
 *     (12-50 % faster on the 64-channel layers); the host mirror uses this form. */
RSLO_API int rslo_weight_transpose(const float *W, int K, int cin, int cout, float *Wt, void *stream);
/*     fp32-accurate sparse conv on the bf16 matrix cores (channel counts 32 / 64): every fp32 value is split exactly
 *     into three bf16 pieces (hi + mid + lo); six bf16 MFMAs (hh, hm, mh, hl, mm, lh) with fp32 accumulation replace
 *     the fp32 MFMAs -- error below one fp32 ulp per product, 2.5x fewer matrix-core cycles.
 *     rslo_weight_split: W [K,Cin_w,Cout_w] fp32 -> Ws (3 planes of bf16, K*cin_op*cout_op each, MFMA operand order);
 *     transpose = 1 gives the operator of the data gradient (cin_op = Cout_w, cout_op = Cin_w).
 *     rslo_spconv_fwd_split == rslo_spconv_fwd with the split weights. */
RSLO_API size_t rslo_weight_split_bytes(int K, int cin, int cout);
RSLO_API int rslo_weight_split(const float *W, int K, int cin_op, int cout_op, int transpose, void *Ws, void *stream);
/*      rslo_weight_split_many: the same split for every 32/64-channel layer of a model, both orientations (forward and
 *      data gradient), in ONE launch -- the weights are constant between optimizer steps.  desc_dev = device array of
 *      n_layers descriptors, max_weight_elems = max over layers of K * cin * cout. */
typedef struct {
  const float *W;   /* [K,cin,cout] */
  void *ws_fwd;     /* rslo_weight_split_bytes(K, cin, cout) bytes: operand of rslo_spconv_fwd_split(x, .., cin, cout) */
  void *ws_dgrad;   /* same size: operand of the data-gradient call rslo_spconv_fwd_split(dout, .., cout, cin) */
  int32_t K, cin, cout;
} RsloWeightSplitDesc;
RSLO_API int rslo_weight_split_many(const RsloWeightSplitDesc *desc_dev, int n_layers, int64_t max_weight_elems,
                                    void *stream);
RSLO_API int rslo_spconv_fwd_split(const float *in, int cin, const void *Ws, const float *bias, const int32_t *nbr,
                                   const int32_t *row_order, int64_t n_out, int K, int cout, int flip_k,
                                   float act_slope, float *out, const int32_t *n_live_dev, void *stream);
/*     Tuning switches of the launch code.  The library reads NO environment variable: tile shapes and kernel variants that
 *     exist for A/B measurements and for the parity tests that pin every tiling against the oracle are set through these
 *     calls (process-wide; the defaults are the measured choices).  Names (rslo_tuning_name(i), i = 0 .. until NULL):
 *     conv2d_wgrad_s2_fullres, conv2d_wgrad_nb, conv2d_wgrad_wgs, conv2d_fwd_tr, conv2d_fwd_mtw, conv2d_fwd_occ,
 *     conv2d_fwd_kc, conv2d_fwd_lean, conv2d_fwd_xsc, conv2d_s2_mtw, conv2d_s2_xsc, bn_small_rc, spconv_rbw, spconv_ks,
 *     spconv_v, spconv_wgrad_split, wgrad_xcd, vfe_lds, chamfer, chamfer_segments, dense_tiled, conv1x1_split, conv2d_fwd_wl
 *     (meanings: csrc/rslo_common.h RsloTune).  Every setting
 *     computes the same products; only tiling, summation grouping and launch geometry change.  Unknown name -> RSLO_EINVAL.
 *     (The reference has no counterpart: spconv / cuDNN pick their algorithms internally.)
 *     spconv_rbw / spconv_ks, the tiling of k_spconv_v6 behind rslo_spconv_fwd_split: a tile is 16*rbw rows (rbw 1, 2, 4) and
 *     ks waves (1, 2, 4) share it, each walking 1/ks of the tile's active kernel offsets; their accumulators are added
 *     through LDS in wave order (a fixed summation order, results within fp32 rounding of the one-wave form).  0 = the
 *     library chooses per layer shape (default: 32 rows and two waves except for 32 -> 32 channels). */
RSLO_API int rslo_tuning_set(const char *name, int value);
RSLO_API int rslo_tuning_get(const char *name, int *value);
RSLO_API const char *rslo_tuning_name(int index);
/*     bf16 feature path (BASELINE config C4: bf16 features, int32 rulebook, fp32 accumulate): in / out are bf16 rows
 *     [N,C], Wb the weights rounded to bf16 in MFMA operand order (rslo_weight_to_bf16, K*cin*cout*2 bytes; transpose
 *     = 1 for the data gradient), bias fp32.  Channel counts 32 / 64. */
RSLO_API int rslo_weight_to_bf16(const float *W, int K, int cin_op, int cout_op, int transpose, void *Wb, void *stream);
RSLO_API int rslo_spconv_fwd_bf16(const void *in, int cin, const void *Wb, const float *bias, const int32_t *nbr,
                                  const int32_t *row_order, int64_t n_out, int K, int cout, int flip_k,
                                  float act_slope, void *out, void *stream);
/*     bf16 feature path, backward: g = dout * act'(y) on bf16 rows (+ per-block column sums of g in fp32, stage 1 of the
 *     bias gradient; partial [rslo_leaky_bwd_colsum_bf16_blocks(rows, cols), cols] or NULL; cols must divide 2048), and
 *     the pair-list weight gradient with bf16 rows on both sides, fp32 accumulation and fp32 dW / dbias (workspace size:
 *     rslo_spconv_wgrad_pairs_ws_bytes; dbias requires bias_partial).  The data gradient is rslo_spconv_fwd_bf16 on the
 *     transposed operand (rslo_weight_to_bf16(..., transpose = 1)). */
RSLO_API int64_t rslo_leaky_bwd_colsum_bf16_blocks(int64_t rows, int cols);
RSLO_API int rslo_leaky_bwd_colsum_bf16(const void *y, const void *dout, int64_t rows, int cols, float slope, void *g,
                                        float *partial, void *stream);
RSLO_API int rslo_spconv_wgrad_pairs_bf16(const void *in, int cin, const void *dout, int cout, const int32_t *pairs_in,
                                          const int32_t *pairs_out, const int32_t *koff, int64_t n_out, int K, void *ws,
                                          size_t ws_bytes, float *dW, float *dbias, const float *bias_partial,
                                          int n_bias_partial, void *stream);
RSLO_API size_t rslo_spconv_wgrad_ws_bytes(int64_t n_out, int K, int cin, int cout);
RSLO_API int rslo_spconv_wgrad(const float *in, int cin, const float *dout, int cout, const int32_t *nbr,
                      int64_t n_out, int K, void *ws, size_t ws_bytes, float *dW /*[K,cin,cout]*/,
                      float *dbias /*[cout] or NULL*/, void *stream);
/* Scheduling order of a neighbour table's rows for rslo_spconv_fwd / _dgrad / _fwd_split / _fwd_bf16: inside every
 * window of 2048 consecutive rows, rows are sorted by their neighbour mask so that the kernels' 16/32-row tiles issue
 * matrix operations for fewer kernel offsets no row of the tile needs.  order [n_rows] is a permutation of 0..n_rows-1
 * (deterministic).  flip_k = 1: order for calls made with flip_k = 1 (SubM data gradient).  Replaces nothing in the
 * reference: spconv's gather-GEMM-scatter walks complete pair lists per offset and has no tile skipping to feed. */
RSLO_API int rslo_rulebook_row_order(const int32_t *nbr, int64_t n_rows, int K, int flip_k, int32_t *order,
                                     void *stream);
/* Pair-list view of a neighbour table (the spconv-1.x rulebook layout): pairs of offset k are contiguous in
 * [koff[k], koff[k+1]) in ascending output row; pairs_in/out need room for n_rows*K entries (upper bound),
 * koff [K+1] lives on the device.  Built once per indice_key; feeds the weight-gradient kernel. */
RSLO_API size_t rslo_rulebook_pairs_ws_bytes(int64_t n_rows, int K);
RSLO_API int rslo_rulebook_pairs(const int32_t *nbr, int64_t n_rows, int K, void *ws, size_t ws_bytes,
                        int32_t *pairs_in, int32_t *pairs_out, int32_t *koff /*[K+1]*/, void *stream);
/* a11 / a12 / a15  The element-wise tail of the BEV head (rslo/models/odom_pred.py:227-264):
 *   rslo_tq_normalize_*   tq_map = cat(t, q / |q|) per cell (odom_pred.py:229-234), tq [B,7,cells];
 *   rslo_conf_softmax_*   both ConfidenceModule softmaxes (rslo/layers/confidence.py:26-34): where(outside, -1000, logit) / T,
 *                         softmax over the cells of a sample; T = 1 -> t_conf, r_conf [B,cells] (with gradient) and
 *                         T = temperature (20) -> conf_temp [B,2,cells] (no gradient) from one pass; outside: 1 byte per cell;
 *   rslo_head_masks_*     occupancy pyramid (mask_gen_pools: MaxPool 3/2/1, odom_pred_base.py:228-231), loss weights
 *                         w_0 = mask * conf_temp, w_{k+1} = occ_{k+1} * AvgPool(3,2,1)(w_k) (hier_weight_gen, odom_pred.py:148,262-264),
 *                         masked pyramid predictions pred_k * (occ_k > 0), masked pose maps tq * mask, tq_g * mask. */
RSLO_API int rslo_tq_normalize_fwd(const float *tq, int B, int64_t cells, float *out, void *stream);
RSLO_API int rslo_tq_normalize_bwd(const float *tq, const float *grad, int B, int64_t cells, float *dtq, void *stream);
RSLO_API int rslo_conf_softmax_fwd(const float *t_logit, const float *r_logit, const unsigned char *outside, int B,
                                   int cells, float temperature, float *t_conf, float *r_conf, float *conf_temp,
                                   void *stream);
RSLO_API int rslo_conf_softmax_bwd(const float *t_conf, const float *r_conf, const float *g_t, const float *g_r,
                                   const unsigned char *outside, int B, int cells, float *d_t_logit, float *d_r_logit,
                                   void *stream);
typedef struct {
  const float *mask;        /* [B,1,H,W] 0/1 */
  const float *conf;        /* [B,2,H,W] */
  const float *tq, *tq_g;   /* [B,7,H,W] */
  const float *pred[3];     /* pred[k-1]: [B,7,H>>k,W>>k], k = 1 .. levels-1 */
  float *w[4];              /* out: w[k] [B,2,H>>k,W>>k] */
  float *occ[4];            /* out: occ[k], k >= 1: [B,1,H>>k,W>>k] */
  float *mpred[3];          /* out: masked predictions */
  float *mtq, *mtq_g;       /* out */
  int32_t B, H, W, levels;  /* levels = 1 + number of pyramid predictions (<= 4) */
} RsloHeadMasks;
typedef struct {
  const float *mask;
  const float *occ[4];
  const float *g_mpred[3];  /* may be NULL */
  const float *g_mtq;       /* may be NULL */
  float *d_pred[3];
  float *d_tq;
  int32_t B, H, W, levels;
} RsloHeadMasksBwd;
RSLO_API int rslo_head_masks_fwd(const RsloHeadMasks *h_a, void *stream);
RSLO_API int rslo_head_masks_bwd(const RsloHeadMasksBwd *h_a, void *stream);
/*     Input of a deblock (odom_pred.py:219-221: deblock(cat([x, skip], 1)) with deblock[0] = nn.Upsample(scale)):
 *     out [B,Ca+Cb,scale*H,scale*W] = nearest-neighbour upsampling of the channel concatenation of a [B,Ca,H,W] and
 *     b [B,Cb,H,W] in one launch; _bwd: da / db (either may be NULL) = the scale x scale window sums of grad, summed in
 *     upsample_nearest2d_backward's order. */
RSLO_API int rslo_cat_upsample_fwd(const float *a, const float *b, int B, int Ca, int Cb, int H, int W, int scale, float *out,
                                   void *stream);
RSLO_API int rslo_cat_upsample_bwd(const float *grad, int B, int Ca, int Cb, int H, int W, int scale, float *da, float *db,
                                   void *stream);
/*     The voted pose odom [B,7] = (t, q) -> t [B,3], r [B,4] = q / (|q| + 1e-12) (odom_pred.py:279-288) and its gradient
 *     (g_t / g_r may be NULL = zeros), one launch each way. */
RSLO_API int rslo_pose_tail_fwd(const float *odom, int B, float *t, float *r, void *stream);
RSLO_API int rslo_pose_tail_bwd(const float *odom, const float *g_t, const float *g_r, int B, float *d_odom, void *stream);

/* a21  Loss assembly in one launch each way: AdaptiveWeightedL2Loss of the voted pose against the ICP pseudo-targets
 *      (rslo/core/losses.py:144-197; mask = ones, focal_gamma = 0), the same reduction of the pyramid levels' per-sample
 *      terms (rslo/models/voxel_odom_net.py:743-798; loss_b from rslo_pyramid_l2_fwd), the consistency loss's reduce over
 *      the per-pair terms (losses.py:496-506) and the weighted total (voxel_odom_net.py:324-376).
 *      out5 = (total, T, R, pyramid, C).  Pointers are device pointers; alpha_* point at the modules' log-variance
 *      parameters (they may alias: the shipped configuration uses the SAME modules for pose and pyramid terms). */
#define RSLO_LOSS_TAIL_MAX_LEVELS 8
#define RSLO_LOSS_TAIL_ALPHA_STRIDE 4
typedef struct {
  const float *t_pred, *t_tgt;        /* [B,3] */
  const float *q_pred, *q_tgt;        /* [B,4] (w,x,y,z) */
  const float *alpha_T, *alpha_R;     /* [1] each */
  const float *pyr_loss_b;            /* [L,B,2] or NULL */
  const float *alpha_pT, *alpha_pR;
  const float *pair_loss;             /* [n_pairs] or NULL */
  const float *alpha_C;
  int32_t B, L, n_pairs, reserved;
  float w_T, w_R, w_pT, w_pR;         /* the modules' _loss_weight */
  float c_scale;                      /* (1 - warm_weight) * prediction weight * consistency _loss_weight */
  float level_w[RSLO_LOSS_TAIL_MAX_LEVELS];   /* pyloss_exp_w_base ** (L - l) */
} RsloLossTail;
RSLO_API int rslo_loss_tail_fwd(const RsloLossTail *h_p, float *out5, void *stream);
RSLO_API int rslo_loss_tail_bwd(const RsloLossTail *h_p, const float *grad_out /*[1]*/, float *d_t /*[B,3]*/,
                                float *d_q /*[B,4]*/, float *d_pyr /*[L,B,2]*/, float *d_pair /*[n_pairs]*/,
                                float *d_alpha5 /*(T, R, pT, pR, C): 5 x RSLO_LOSS_TAIL_ALPHA_STRIDE floats*/, void *stream);
/*     d_alpha5: entry i is written to d_alpha5[i * RSLO_LOSS_TAIL_ALPHA_STRIDE] -- 16-byte slots, so that each one can be
 *     handed on as a parameter's gradient tensor (the optimizer's tables take 16-byte aligned gradients).  A module that
 *     serves several terms (the same alpha pointer more than once): its FIRST entry holds the sum of all of them, added in
 *     entry order. */

/* ------------------------------------------------------------------------------------
 * a1 + a2 + a5 in ONE call: voxelization of all clouds of a step (frames x samples) and the complete rulebook chain
 * of a chain-structured sparse encoder -- site hashes, SubM tables, strided-conv output sets + both tables, tile row
 * orders, weight-gradient pair lists -- without a host read.  Replaces, for a whole training step, the DataLoader-side
 * VoxelGenerator.generate calls + merge_second_batch coordinate padding (rslo/data/preprocess.py:493,75-89) and the
 * implicit indice-pair builds of SpMiddleFHDWithCov2_3 (rslo/models/middle.py:119-213, keys subm0 .. dsubm1).
 *
 * Levels: level 0 = the voxel grid (dims0 = sparse_shape, z y x); level l+1 = output of the strided conv l
 * (conv_ks/stride/pad[l]); subm_ks[l] != 0 asks for the SubM table of level l.  Batch index of cloud c in the batched
 * encoder tensor = c (clouds are given frame-major: c = t * clouds_per_frame + b); its index inside its frame = b.
 * Everything lives in ONE caller-owned arena (rslo_plan_encoder_layout gives the offsets; capacities instead of exact
 * sizes: level 0 = min(n_clouds * max_voxels, sum P), level l+1 = capacity of level l unless cap_rows[] says otherwise).
 * Actual sizes are device words in the counts block, copied asynchronously to h_counts (pinned host memory, may be
 * NULL) at the end; the caller reads them after synchronising with an event recorded behind the call:
 *   counts[RSLO_PLAN_CNT_OVERFLOW]      bit l set: level l had more sites than its capacity (rows past it dropped:
 *                                       the plan is unusable, re-plan with larger cap_rows)
 *   counts[RSLO_PLAN_CNT_ROWS + l]      active sites of level l
 *   counts[RSLO_PLAN_CNT_NVOX + c]      voxels of cloud c
 *   counts[RSLO_PLAN_CNT_BOFF + l*(RSLO_PLAN_MAX_CLOUDS+1) + j]   first row of batch element j on level l (j = 0..n)
 * Results equal the stand-alone entry points above bit for bit (same kernels, row counts read from the device).
 * ------------------------------------------------------------------------------------ */
#define RSLO_PLAN_MAX_LEVELS 8
#define RSLO_PLAN_MAX_CLOUDS 64
#define RSLO_PLAN_CNT_OVERFLOW 0
#define RSLO_PLAN_CNT_ROWS 1
#define RSLO_PLAN_CNT_RAW 9
#define RSLO_PLAN_CNT_NVOX 32
#define RSLO_PLAN_CNT_BASE 96
#define RSLO_PLAN_CNT_BOFF 176
#define RSLO_PLAN_CNT_WORDS (176 + RSLO_PLAN_MAX_LEVELS * (RSLO_PLAN_MAX_CLOUDS + 1))
typedef struct {
  int32_t n_levels;
  int32_t dims0[3];                              /* sparse_shape (z, y, x) of level 0 */
  int32_t subm_ks[RSLO_PLAN_MAX_LEVELS][3];      /* 0,0,0: no SubM table on this level */
  int32_t conv_ks[RSLO_PLAN_MAX_LEVELS][3], conv_stride[RSLO_PLAN_MAX_LEVELS][3], conv_pad[RSLO_PLAN_MAX_LEVELS][3];
  int32_t want_pairs, want_orders;               /* want_orders: bit l = a mask-sorted row order for the transposed table of level l's strided conv */
  float range6[6], vsize3[3];                    /* voxelizer geometry (rslo_voxelize) */
  int32_t grid_xyz[3], max_points, max_voxels, n_features;
  int64_t cap_rows[RSLO_PLAN_MAX_LEVELS];        /* 0 = default capacity */
} RsloEncoderSpec;
typedef struct {
  uint64_t total_bytes;
  int32_t dims[RSLO_PLAN_MAX_LEVELS][3];
  int64_t cap_rows[RSLO_PLAN_MAX_LEVELS], hash_cap[RSLO_PLAN_MAX_LEVELS];
  uint64_t counts_off;                           /* int32 [RSLO_PLAN_CNT_WORDS] */
  uint64_t voxels_off, num_points_off;           /* fp32 [cap0, T, F], int32 [cap0]: all clouds, frame-major */
  uint64_t coords_frame_off;                     /* int32 [cap0, 4]: (index inside the frame, z, y, x) */
  uint64_t coords_off[RSLO_PLAN_MAX_LEVELS];     /* int32 [cap_l, 4]: (batch, z, y, x); level 0 = all clouds */
  uint64_t keys_off[RSLO_PLAN_MAX_LEVELS], vals_off[RSLO_PLAN_MAX_LEVELS];
  uint64_t subm_nbr_off[RSLO_PLAN_MAX_LEVELS], subm_pin_off[RSLO_PLAN_MAX_LEVELS], subm_pout_off[RSLO_PLAN_MAX_LEVELS],
      subm_koff_off[RSLO_PLAN_MAX_LEVELS];
  uint64_t conv_nbr_off[RSLO_PLAN_MAX_LEVELS], conv_nbrT_off[RSLO_PLAN_MAX_LEVELS], conv_order_off[RSLO_PLAN_MAX_LEVELS],
      conv_pin_off[RSLO_PLAN_MAX_LEVELS], conv_pout_off[RSLO_PLAN_MAX_LEVELS], conv_koff_off[RSLO_PLAN_MAX_LEVELS];
  int64_t scratch_words;
  uint64_t vox_ws_off, bitmap_off, prefix_off, scan_ws_off, pair_ws_off;
  uint64_t keys_end_off;                                 /* keys_off[0] .. keys_end_off: the keys of all levels (one fill) */
  uint64_t bitmap_level_off[RSLO_PLAN_MAX_LEVELS], bitmap_end_off;   /* output bitmap of conv l, all levels contiguous */
} RsloPlanLayout;
RSLO_API int rslo_plan_encoder_layout(const RsloEncoderSpec *h_spec, int n_clouds, const int64_t *h_n_points,
                                      RsloPlanLayout *h_layout);
RSLO_API int rslo_plan_encoder(const RsloEncoderSpec *h_spec, const RsloPlanLayout *h_layout, int n_clouds,
                               int clouds_per_frame, const float *const *h_points /*n_clouds device pointers [P,F]*/,
                               const int64_t *h_n_points, void *arena, size_t arena_bytes,
                               int32_t *h_counts /*pinned, [RSLO_PLAN_CNT_WORDS] or NULL*/, void *stream);

/*     rslo_plan_encoder_pad_tails (round 5): behind rslo_plan_encoder on the same stream, turns the rows of every table past
 *     its level's device-side count -- up to the level's CAPACITY -- into padding rows: coordinates -1 (rslo_dense_scatter
 *     skips them), neighbour entries -1 (a padding output row gathers nothing), tile orders continued as the identity.  The
 *     encoder's kernels can then be launched for capacity-sized tensors whose shapes do not depend on the scan: what an
 *     inference loop needs to replay ONE hipGraph per arena (evaluate.py:363-408 runs the same forward frame after frame). */
RSLO_API int rslo_plan_encoder_pad_tails(const RsloEncoderSpec *h_spec, const RsloPlanLayout *h_layout, void *arena,
                                         void *stream);

/* wgrad over pair lists: dW[k] = sum_{p in [koff[k],koff[k+1])} in[pairs_in[p]]^T dout[pairs_out[p]];
 * dbias = column sums of dout (all n_out rows).  Deterministic (fixed-order two-stage reduction). */
RSLO_API size_t rslo_spconv_wgrad_pairs_ws_bytes(int64_t n_out, int K, int cin, int cout);
RSLO_API int rslo_spconv_wgrad_pairs(const float *in, int cin, const float *dout, int cout, const int32_t *pairs_in,
                            const int32_t *pairs_out, const int32_t *koff, int64_t n_out, int K, void *ws,
                            size_t ws_bytes, float *dW /*[K,cin,cout]*/, float *dbias /*[cout] or NULL*/,
                            const float *bias_partial /*[n_bias_partial,cout] from rslo_leaky_bwd_colsum, or NULL*/,
                            int n_bias_partial, void *stream);
/* LeakyReLU backward from the saved OUTPUT (sign-preserving): g = dout * (y > 0 ? 1 : slope). */
RSLO_API int rslo_leaky_bwd(const float *y, const float *dout, int64_t n, float slope, float *g, void *stream);
/*     The same plus per-block column sums of g (stage 1 of the bias gradient; cols must divide 1024):
 *     partial [rslo_leaky_bwd_colsum_blocks(rows, cols), cols] is handed to rslo_spconv_wgrad_pairs. */
RSLO_API int64_t rslo_leaky_bwd_colsum_blocks(int64_t rows, int cols);
RSLO_API int rslo_leaky_bwd_colsum(const float *y, const float *dout, int64_t rows, int cols, float slope, float *g,
                                   float *partial, void *stream);

/* a7  Per-frame BatchNorm1d (+ fused LeakyReLU) of the covariance branch (nn.BatchNorm1d at
 *     rslo/models/middle.py:181-198; the reference feeds one frame per call, so statistics are per frame).
 * Rows are grouped by frame: seg_off [S+1] (device).  Training-mode semantics of S consecutive module calls:
 * biased variance for normalisation, running estimates updated in segment order with the unbiased variance.
 * y = act(gamma * (x - mean_s) * invstd_s + beta); save_mean / save_invstd [S,C] feed the backward. */
RSLO_API size_t rslo_segbn_ws_bytes(int S, int64_t max_seg_len, int C);
RSLO_API int rslo_segbn_fwd(const float *x, int C, const int32_t *seg_off, int S, int64_t max_seg_len,
                   const float *gamma, const float *beta, float *running_mean /*or NULL*/,
                   float *running_var /*or NULL*/, float momentum, float eps, float act_slope, void *ws,
                   size_t ws_bytes, float *y, float *save_mean, float *save_invstd, void *stream);
/*     Eval mode (evaluate.py:363-408; the nn.BatchNorm1d layers of rslo/models/middle.py:181-213 with their running statistics):
 *     y = act((x - running_mean) / sqrt(running_var + eps) * gamma + beta) over [n, C] rows in one launch; act_slope 1 = no
 *     activation; gamma / beta may be NULL; n_live_dev (or NULL): device count of the live rows (rows past it stay unwritten). */
RSLO_API int rslo_bn1d_eval_act(const float *x, int64_t n, int C, const float *running_mean, const float *running_var,
                                const float *gamma, const float *beta, float eps, float act_slope, const int32_t *n_live_dev,
                                float *y, void *stream);
/* ws_bytes >= rslo_segbn_ws_bytes(...) + 2*S*C*4 */
RSLO_API int rslo_segbn_bwd(const float *x, const float *y, const float *gy, int C, const int32_t *seg_off, int S,
                   int64_t max_seg_len, const float *gamma, const float *save_mean, const float *save_invstd,
                   float act_slope, void *ws, size_t ws_bytes, float *gx, float *dgamma, float *dbeta,
                   void *stream);

/* a8  SparseConvTensor.dense() + view (middle.py:240-243): [M,C] rows -> [B,C,D,H,W]
 *     (zero-filled here) and its backward gather. */
RSLO_API int rslo_dense_scatter(const float *feat, const int32_t *coords, int64_t M, int C, int B,
                       const int32_t *h_dims3, float *out, void *stream);
RSLO_API int rslo_dense_gather(const float *dense, const int32_t *coords, int64_t M, int C, int B,
                      const int32_t *h_dims3, float *dfeat, void *stream);
/*     The same with the frames of a sample side by side: the batch holds frame t of sample b at index t * (B / frames) + b
 *     and the dense tensor is [B / frames, frames, C, D, H, W] = the channel concatenation the BEV head builds from a
 *     pair's frames (rslo/models/odom_pred.py:170, odom_pred_base.py:305-324), produced without a copy. */
RSLO_API int rslo_dense_scatter_frames(const float *feat, const int32_t *coords, int64_t M, int C, int B, int frames,
                                       const int32_t *h_dims3, float *out, void *stream);
RSLO_API int rslo_dense_gather_frames(const float *dense, const int32_t *coords, int64_t M, int C, int B, int frames,
                                      const int32_t *h_dims3, float *dfeat, void *stream);
/*     Per-cell sums over each of the G channel groups of a BEV tensor [B, G*Cg, HW] -> [B, G, HW] in one pass: feeds the
 *     occupancy masks (odom_pred.py:165-168; voxel_odom_net.py:519-527) and the logged channel means. */
RSLO_API int rslo_bev_channel_sums(const float *in, int B, int G, int Cg, int64_t HW, float *out, void *stream);
/*     The same pass also writing the occupancy of channel group 0 in the three forms the head uses (odom_pred.py:165-168 and
 *     rslo/layers/confidence.py:26-34): mask_f [B,HW] float 0/1, mask_b [B,HW] bytes 0/1, outside_b = !mask_b.  Any may be NULL. */
RSLO_API int rslo_bev_channel_sums_masks(const float *in, int B, int G, int Cg, int64_t HW, float *out, float *mask_f,
                                         unsigned char *mask_b, unsigned char *outside_b, void *stream);
/*     The logged extras from those sums [B,T,HW] in two launches (voxel_odom_net.py:455-464; ws: rslo_bev_display_ws_bytes(T) bytes of partial extrema): mask [B,HW] = (sum over t) != 0;
 *     disp [T,B,HW] = the per-frame channel mean sums / Cg, min-max normalised over the frame's batch
 *     ((d - min) / (max - min + 1e-12)) -- `middle_feature` and `feature_mask` of the training forward. */
RSLO_API size_t rslo_bev_display_ws_bytes(int T);
RSLO_API int rslo_bev_display(const float *sums, int B, int T, int Cg, int64_t HW, float *mask, float *disp, void *ws,
                              size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * a17  Chamfer nearest neighbour.  Replaces cd.forward_cuda_one_direction /
 *      cd.backward_cuda_one_direction (thirdparty/chamfer_distance/chamfer_distance.cpp:62-76,
 *      94-113; kernels chamfer_distance.cu:6-137,177-206).  Arithmetic follows the CPU
 *      nnsearch (chamfer_distance.cpp:116-144): fp32 products and sums without contraction,
 *      strict '<' so the lowest index wins ties -- bit-exact dist and idx vs that path.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_chamfer_ws_bytes(int B, int N, int M);
RSLO_API int rslo_chamfer_nn(const float *xyz1 /*[B,N,3]*/, const float *xyz2 /*[B,M,3]*/, int B, int N, int M,
                    float *dist /*[B,N]*/, int32_t *idx /*[B,N]*/, void *ws, size_t ws_bytes,
                    void *stream);
/* Ragged batch: pair b uses only its first ncnt[b] queries and mcnt[b] targets of the padded [B,N,3]/[B,M,3]
 * arrays (device int32 [B]; NULL = all).  Padding queries get dist = +inf, idx = 0. */
RSLO_API int rslo_chamfer_nn_ragged(const float *xyz1, const float *xyz2, int B, int N, int M, const int32_t *ncnt,
                           const int32_t *mcnt, float *dist, int32_t *idx, void *ws, size_t ws_bytes,
                           void *stream);
/*     Exact search with spatial pruning (Morton bucket sort of both clouds, 64-point target tiles with bounding
 *     boxes, box lower bound in the distance's own operation order => bit-identical to the exhaustive scan).
 *     rslo_chamfer_nn / _ragged dispatch to it for N >= 1024 and M >= 2048 (tuning switch `chamfer`: 1 = exhaustive, 2 = pruned);
 *     rslo_chamfer_ws_bytes covers both. */
RSLO_API int rslo_chamfer_brute_nn(const float *xyz1, const float *xyz2, int B, int N, int M, const int32_t *ncnt,
                                   const int32_t *mcnt, float *dist, int32_t *idx, void *ws, size_t ws_bytes,
                                   void *stream);   /* the exhaustive scan, explicitly */
RSLO_API size_t rslo_chamfer_grid_ws_bytes(int B, int N, int M);
RSLO_API int rslo_chamfer_grid_nn(const float *xyz1, const float *xyz2, int B, int N, int M, const int32_t *ncnt,
                                  const int32_t *mcnt, float *dist, int32_t *idx, void *ws, size_t ws_bytes,
                                  void *stream);
RSLO_API int rslo_chamfer_grad(const float *xyz1, const float *xyz2, int B, int N, int M,
                      const float *graddist1, const int32_t *idx1, float *gradxyz1 /*[B,N,3]*/,
                      float *gradxyz2 /*[B,M,3]*/, void *stream);

/* ------------------------------------------------------------------------------------
 * a18-a20  Consistency loss (rslo/core/losses.py:337-507, Aleat5_1ChamferL2NormalWeightedALLSVDLoss).
 * All arrays are per frame pair b in [0,B): p1 [B,N,3] source voxel means, n1 [B,N,3] their normals,
 * tgt [B,M,3] posed target means, cov1 [B,N,7] / cov2 [B,M,7] covariance parameters
 * (3 eigenvalue increments + quaternion read as x,y,z,w -- losses.py:348-363), idx/dist [B,N] the
 * chamfer association, thr [B] = max(kth(dist), 1) (losses.py:326-334), Rd [B,9] the detached pose.
 *
 * cov_residual_fwd: loss[b] = mean_roi(d^T sigma^-1 d) + reg * mean_roi(0.5 log det sigma),
 *                   sigma = S1 + Rd S2[idx] Rd^T, d = p1 - tgt[idx], roi = dist < thr (losses.py:396-435;
 *                   closed-form 3x3 inverse/det instead of torch.inverse/torch.det over ~30k matrices).
 * cov_residual_bwd: gradients of sum_b gloss[b]*loss[b] w.r.t. tgt, cov1, cov2 (and p1 if gp1 != NULL).
 * icp_step        : one SVDHead refinement (rslo/layers/svd.py:14-64 called from losses.py:451-465):
 *                   weighted Kabsch over the ROI with w = cos(n1, tgt[idx]-p1)^2, unweighted centroids,
 *                   reflection fix, returns the inverse motion and composes res_r = R res_r,
 *                   res_t = R res_t + t in place.  No host round trip (the reference branches on det(R)).
 * transform_points: out = R x + t per pair (losses.py:471-473).
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_cov_residual_ws_bytes(int B, int N);
RSLO_API int rslo_cov_residual_fwd(const float *p1, const float *tgt, const float *cov1, const float *cov2,
                          const int32_t *idx, const float *dist, const float *thr, const float *Rd, int B, int N,
                          int M, float reg_weight, void *ws, size_t ws_bytes, float *loss /*[B]*/,
                          float *cnt /*[B]*/, void *stream);
RSLO_API int rslo_cov_residual_bwd(const float *p1, const float *tgt, const float *cov1, const float *cov2,
                          const int32_t *idx, const float *dist, const float *thr, const float *Rd,
                          const float *gloss /*[B]*/, const float *cnt /*[B]*/, int B, int N, int M,
                          float reg_weight, float *gp1 /*[B,N,3] or NULL*/, float *gtgt /*[B,M,3]*/,
                          float *gcov1 /*[B,N,7]*/, float *gcov2 /*[B,M,7]*/, void *ws, size_t ws_bytes, void *stream);
/*     The gradients that land on the PARTNER rows (gtgt, gcov2: several sources may share a partner) are added in ascending
 *     source order: every source leaves its ten values and the key (partner row, source row), the keys are sorted (radix
 *     sort over B N 64-bit keys) and each partner's run is added by one thread (runs of up to 32 sources) or one wave
 *     (fixed lane assignment + fixed tree) -- bit-reproducible from run to run, where per-run atomics (rounds 1-4, deleted in
 *     round 6) made every training step unique.  ws: rslo_cov_residual_bwd_ws_bytes(B, N, M). */
RSLO_API size_t rslo_cov_residual_bwd_ws_bytes(int B, int N, int M);
RSLO_API size_t rslo_icp_ws_bytes(int B, int N);
RSLO_API int rslo_icp_step(const float *p1, const float *n1, const float *tgt, const int32_t *idx, const float *dist,
                  const float *thr, int B, int N, int M, void *ws, size_t ws_bytes, float *res_r /*[B,9] in/out*/,
                  float *res_t /*[B,3] in/out*/, float *step_R /*[B,9] or NULL*/, float *step_t /*[B,3] or NULL*/,
                  void *stream);
/*     _first: the first refinement of a pair -- res_r / res_t are outputs only (the running motion starts as the identity,
 *     losses.py:452-453), the caller does not fill them. */
RSLO_API int rslo_icp_step_first(const float *p1, const float *n1, const float *tgt, const int32_t *idx, const float *dist,
                  const float *thr, int B, int N, int M, void *ws, size_t ws_bytes, float *res_r /*[B,9] out*/,
                  float *res_t /*[B,3] out*/, float *step_R /*[B,9] or NULL*/, float *step_t /*[B,3] or NULL*/,
                  void *stream);
/* a18  ROI threshold (rslo/core/losses.py:326-334): thr[b] = max(k-th smallest of dist[b][0..counts[b]), 1) with
 *      k = 1 + int(counts[b] * ratio); counts NULL = N everywhere.  Exact (radix select), no sort. */
RSLO_API int rslo_roi_threshold(const float *dist, int B, int N, const int32_t *counts, double ratio, float *thr,
                                void *stream);
RSLO_API int rslo_transform_points(const float *x, const float *R, const float *t, int B, int M, float *out,
                          void *stream);
/*     The same rigid map on rows of `row_stride` floats (t may be NULL), and its pose gradient
 *     dR[b] = sum_j g[b][j] x[b][j]^T, dt[b] = sum_j g[b][j]  (p2_moved / n2_moved of the loss assembly,
 *     rslo/models/voxel_odom_net.py:668-676).  done: int32 [B] counters, zero on entry, left zero. */
RSLO_API int rslo_transform_rows(const float *x, int row_stride, const float *R, const float *t, int B, int M,
                                 float *out, void *stream);
RSLO_API size_t rslo_transform_rows_bwd_ws_bytes(int B, int M);
RSLO_API int rslo_transform_rows_bwd(const float *x, int row_stride, const float *gout, int B, int M, void *ws,
                                     size_t ws_bytes, int32_t *done, float *dR, float *dt, void *stream);

/* a21  pyramid supervision of the per-cell local transformation maps, all levels in one launch
 *      (rslo/models/voxel_odom_net.py:706-760 pyramid part of create_loss; target map of gen_tq_maps
 *      voxel_odom_net.py:575-600 = generate_pointwise_local_transformation_tch rslo/data/dataset.py:118-168,
 *      nearest-resampled per level by F.interpolate; per-sample masked L2 of AdaptiveWeightedL2Loss
 *      rslo/core/losses.py:144-197).
 *      level l: pred [B,7,h,w] (t_l xyz, q wxyz), mask [B,Cm,h,w] (channel 0 weighs the translation part,
 *      channel Cm-1 the rotation part).  tq [B,7] = global pose targets (t, q wxyz).  The target of a cell is
 *      t_l = R(q)^-1 (t_g - x) + x with x the centre of the nearest cell of the H0 x W0 map.
 *      loss_b [L,B,2] = sum(diff^2 mask) / (n_ch sum(mask) + 1e-12) for (T, R);  den [L,B,2] = n_ch sum(mask).
 *      done: [L*B] int32 counters, zero on entry, left zero on exit.  bwd writes levels[l].dpred [B,7,h,w]. */
typedef struct {
  const float *pred;
  const float *mask;
  float *dpred;          /* bwd only */
  int32_t h, w, mask_channels;
} RsloPyramidLevel;
RSLO_API size_t rslo_pyramid_l2_ws_bytes(const RsloPyramidLevel *h_levels, int n_levels, int B);
RSLO_API int rslo_pyramid_l2_fwd(const RsloPyramidLevel *h_levels, int n_levels, int B, const float *tq, int H0,
                                 int W0, const float *h_origin3, const float *h_vsize3, void *ws, size_t ws_bytes,
                                 int32_t *done, float *loss_b, float *den, void *stream);
RSLO_API int rslo_pyramid_l2_bwd(const RsloPyramidLevel *h_levels, int n_levels, int B, const float *tq, int H0,
                                 int W0, const float *h_origin3, const float *h_vsize3, const float *grad_loss_b,
                                 const float *den, void *stream);

/* a20  ragged batch assembly of the consistency loss (rslo/models/voxel_odom_net.py:629-651: each sample's frames are
 *      truncated to the shortest; all samples of one frame are gathered into ONE zero-padded batch):
 *      out[b, r, :] = r < len[b] ? src[off[b] + r, :] : 0   (src [N,C], out [B,Lmax,C]);  bwd is the inverse copy,
 *      rows of src outside every [off[b], off[b]+len[b]) get 0.  off/len: int32 [B] on the device. */
RSLO_API int rslo_pad_rows_fwd(const float *src, int64_t N, int C, const int32_t *off, const int32_t *len, int B,
                               int Lmax, float *out, void *stream);
RSLO_API int rslo_pad_rows_bwd(const float *dout, int64_t N, int C, const int32_t *off, const int32_t *len, int B,
                               int Lmax, float *dsrc, void *stream);
/*      rslo_pair_rows_fwd: the three operands of one frame in one launch (voxel_odom_net.py:630-660 selects the xyz and
 *      normal columns of the voxel features, joins them with the covariance head's rows and pads): feats [N,F] (F = 7:
 *      xyz, intensity, normal -- or F = 6: xyz, normal), conf [N,Cc] -> xyz [B,Lmax,3], nrm [B,Lmax,3], cov [B,Lmax,Cc],
 *      zero padded as above.  Only conf carries a gradient: rslo_pad_rows_bwd with C = Cc is its backward. */
RSLO_API int rslo_pair_rows_fwd(const float *feats, int64_t N, int F, const float *conf, int Cc, const int32_t *off,
                                const int32_t *len, int B, int Lmax, float *xyz, float *nrm, float *cov, void *stream);

/* a10-a12  training-mode (Sync)BatchNorm2d of the dense head fused with activation and residual add, NCHW fp32
 *      (apex.parallel.SyncBatchNorm via rslo/layers/SparseConv.py:96-113; rslo/models/custom_resnet_spc.py:224-298).
 *      stats [2C+1] doubles = per-channel sum, sum of squares, element count: the caller all-reduces them across ranks
 *      between rslo_bn2d_stats and rslo_bn2d_apply (nothing to do on one rank).  apply: y = act(gamma (x-mean) invstd +
 *      beta (+ res)), running statistics updated with `momentum` (unbiased variance), mean / invstd saved.
 *      backward: rslo_bn2d_bwd_reduce gives red [2C] = sum g, sum g x^ (g = dy act'(y); all-reduce across ranks) and
 *      the LOCAL dgamma / dbeta; rslo_bn2d_bwd_apply gives dx (and dres = g).  done: int32 [C], zero on entry / exit. */
RSLO_API size_t rslo_bn2d_ws_bytes(int N, int C, int HW);
RSLO_API int rslo_bn2d_stats(const float *x, int N, int C, int HW, void *ws, size_t ws_bytes, int32_t *done,
                             double *stats, void *stream);
RSLO_API int rslo_bn2d_apply(const float *x, const float *res, const double *stats, const float *gamma,
                             const float *beta, int N, int C, int HW, float eps, float momentum, float act_slope,
                             float *running_mean, float *running_var, float *save_mean, float *save_invstd, float *y,
                             void *stream);
RSLO_API int rslo_bn2d_bwd_reduce(const float *dy, const float *y, const float *x, const float *save_mean,
                                  const float *save_invstd, int N, int C, int HW, float act_slope, int has_act,
                                  void *ws, size_t ws_bytes, int32_t *done, double *red, float *dgamma, float *dbeta,
                                  void *stream);
RSLO_API int rslo_bn2d_bwd_apply(const float *dy, const float *y, const float *x, const float *gamma,
                                 const float *save_mean, const float *save_invstd, const double *red, double count,
                                 const double *count_dev /* or NULL: element count over all ranks on the device, e.g.
                                 &stats[2C] after the forward all-reduce (uneven per-rank batches); overrides count */,
                                 int N, int C, int HW, float act_slope, int has_act, float *dx, float *dres,
                                 void *stream);

/*      Single-rank forms (no statistics exchange): statistics slices + apply in two launches, the apply kernels add
 *      the slice partials themselves.  Same results as stats -> apply / bwd_reduce -> bwd_apply with one rank. */
RSLO_API int rslo_bn2d_fwd_local(const float *x, const float *res, const float *gamma, const float *beta, int N, int C,
                                 int HW, float eps, float momentum, float act_slope, float *running_mean,
                                 float *running_var, float *save_mean, float *save_invstd, float *y, void *ws,
                                 size_t ws_bytes, void *stream);
RSLO_API int rslo_bn2d_bwd_local(const float *dy, const float *y, const float *x, const float *gamma,
                                 const float *save_mean, const float *save_invstd, int N, int C, int HW,
                                 float act_slope, int has_act, float *dx, float *dres, float *dgamma, float *dbeta,
                                 void *ws, size_t ws_bytes, void *stream);

/* a13 / a14  local -> global transformation of every BEV cell + confidence-weighted ego-motion vote
 *      (from_pointwise_local_transformation_tch rslo/data/dataset.py:121-208, rotate_vec_by_q
 *       rslo/utils/pose_utils.py:130-142, aggregate_tq rslo/models/odom_pred.py:347-357).
 *      tq_map [B,7,H,W] (t_l xyz, q wxyz), t_conf / r_conf [B,1,H,W]  ->  tq_map_g [B,7,H,W], odom [B,7] (t, q),
 *      sums [B,2] = (sum t_conf + 1e-12, sum r_conf + 1e-12).  bwd: gradient of odom -> d tq_map, d t_conf, d r_conf
 *      (tq_map_g carries no gradient on this path).  done: int32 [B], zero on entry / exit. */
RSLO_API size_t rslo_vote_ws_bytes(int B, int H, int W);
RSLO_API int rslo_vote_fwd(const float *tq_map, const float *t_conf, const float *r_conf, int B, int H, int W,
                           const float *h_origin3, const float *h_vsize3, void *ws, size_t ws_bytes, int32_t *done,
                           float *tq_map_g, float *odom, float *sums, void *stream);
RSLO_API int rslo_vote_bwd(const float *tq_map, const float *t_conf, const float *r_conf, int B, int H, int W,
                           const float *h_origin3, const float *h_vsize3, const float *odom, const float *sums,
                           const float *g_odom, float *d_tq_map, float *d_t_conf, float *d_r_conf, void *stream);

/* a10 - a12  weight gradient of the BEV head's dense 3x3 convolutions (torch.nn.Conv2d / MaskConv.conv1 built in
 *      rslo/models/odom_pred.py:65-134,398-426 and rslo/models/custom_resnet_spc.py:224-298; in the reference the
 *      gradient comes from cuDNN through autograd).  NCHW fp32, kernel 3x3, padding 1, stride 1 or 2, cin % 16 == 0,
 *      cout % 32 == 0:  dW [cout,cin,3,3] = sum over batch and output pixels of dout [B,cout,Ho,Wo] x shifted
 *      in [B,cin,H,W].  bf16 matrix cores on exactly split fp32 operands, fixed summation order (no atomics).
 *      rslo_conv2d_wgrad_supported returns 1 for shapes the kernel takes (others stay on the library path).
 *      dbias [cout] (optional, stride 1 only): the bias gradient = per-channel sum of dout, from the same pass. */
RSLO_API int rslo_conv2d_wgrad_supported(int cin, int cout, int H, int W, int stride);
RSLO_API size_t rslo_conv2d_wgrad_ws_bytes(int B, int cin, int cout, int H, int W, int stride);
RSLO_API int rslo_conv2d_wgrad(const float *in, const float *dout, int B, int cin, int cout, int H, int W, int stride,
                               float *dW, float *dbias, void *ws, size_t ws_bytes, void *stream);

/* a10 - a12  forward and data gradient of the same layers (3x3, stride 1, padding 1, NCHW fp32; channels % 32 == 0):
 *      out[b][m] = bias[m] + sum_k A[m][k] (*) in[b][k].  rslo_conv2d_wsplit turns the layer's weight W [cout,cin,3,3]
 *      into split-bf16 MFMA operands: transpose = 0 for the forward pass (m = cout, k = cin), transpose = 1 for the
 *      data gradient (m = cin, k = cout, taps flipped; pass dout as `in`).  rslo_conv2d_fwd's cin / cout are the
 *      contraction / produced channel counts of THAT call.  bias may be NULL. */
RSLO_API int rslo_conv2d_fwd_supported(int cin, int cout, int H, int W);
RSLO_API size_t rslo_conv2d_wsplit_bytes(int cin, int cout);
RSLO_API int rslo_conv2d_wsplit(const float *W, int cin, int cout, int transpose, void *Ws, void *stream);
/*      rslo_conv2d_wsplit_many: the same split for all layers of a model, both orientations, in ONE launch (the weights
 *      are constant between optimizer steps): desc_dev = device array of n_layers descriptors, max_weight_elems =
 *      max over layers of cin * cout * 9. */
typedef struct {
  const float *W;   /* [cout,cin,3,3] */
  void *ws_fwd;     /* rslo_conv2d_wsplit_bytes(cin, cout) bytes, transpose = 0 */
  void *ws_dgrad;   /* same size, transpose = 1 */
  int32_t cin, cout;
  int32_t ntap;     /* 9 (or 0): 3x3 weight; 1: 1x1 weight (operand of rslo_conv2d_fwd_s2 / _dgrad_s2 with ksize 1) */
  int32_t reserved;
} RsloConv2dSplitDesc;
RSLO_API int rslo_conv2d_wsplit_many(const RsloConv2dSplitDesc *desc_dev, int n_layers, int64_t max_weight_elems,
                                     void *stream);
RSLO_API int rslo_conv2d_fwd(const float *in, const void *Ws, const float *bias, int B, int cin, int cout, int H, int W,
                             float *out, void *stream);
/*      rslo_conv2d_fwd_add: out = conv + bias + res, res [B,cout,H,W] read in the epilogue -- the data gradient of a
 *      BasicBlock's first convolution plus the gradient of its identity branch (custom_resnet_spc.py:74-96 backward),
 *      the same bits as the convolution followed by a separate element-wise add.  res must not alias out. */
RSLO_API int rslo_conv2d_fwd_add(const float *in, const void *Ws, const float *bias, const float *res, int B, int cin,
                                 int cout, int H, int W, float *out, void *stream);
/*      Operand planes (round 5).  A dense activation [B,C,H,W] fp32 (C % 8 == 0) stored ONCE, by its producer, in the
 *      form the convolution's MFMA operands have:  P[b][C/8][3 = hi|mid|lo][H][W][8] bf16 bit patterns, hi + mid + lo ==
 *      the fp32 value exactly (the split k_conv2d_fwd performs per workgroup while staging).  rslo_opl_bytes: size of P;
 *      rslo_opl_from_nchw: the stand-alone producer; the BatchNorm apply entry points with a `planes` argument write the
 *      same layout from their epilogue.  rslo_conv2d_fwd_p = rslo_conv2d_fwd / _fwd_add reading P instead of the fp32
 *      tensor (Ws with transpose = 1 and the planes of dout: the data gradient): same arithmetic, bit-identical
 *      results, no operand split and no strided loads in the convolution.  Replaces the same reference calls:
 *      nn.Conv2d inside rslo/layers/MaskConv.py:30-63 as used by custom_resnet_spc.py:224-298 and
 *      rslo/models/odom_pred_base.py:155-207. */
RSLO_API size_t rslo_opl_bytes(int B, int C, int H, int W);
RSLO_API int rslo_opl_from_nchw(const float *in, int B, int C, int H, int W, void *planes, void *stream);
RSLO_API int rslo_conv2d_fwd_p_supported(int cin, int cout, int H, int W);
RSLO_API int rslo_conv2d_fwd_p(const void *planes, const void *Ws, const float *bias, const float *res /* or NULL */,
                               int B, int cin, int cout, int H, int W, float *out, void *stream);
/*      The stride-2 layers of the BEV encoder (first 3x3 convolution and 1x1 downsample of every stage,
 *      rslo/models/odom_pred.py:398-426): ksize 3 (padding 1) or 1 (padding 0), no bias (the reference builds them
 *      bias-free in front of a BatchNorm).  in [B,cin,H,W] -> out [B,cout,Ho,Wo], Ho = (H - 1) / 2 + 1.
 *      rslo_conv2d_wsplit_k: the split operand of a [cout,cin,ksize,ksize] weight (transpose = 1: data gradient);
 *      rslo_conv2d_dgrad_s2 writes every element of din [B,cin,H,W] (per output parity class: no zero-stuffing,
 *      no atomics). */
RSLO_API int rslo_conv2d_s2_supported(int cin, int cout, int ksize);
RSLO_API int rslo_conv2d_wsplit_k(const float *W, int cin, int cout, int ksize, int transpose, void *Ws, void *stream);
RSLO_API int rslo_conv2d_fwd_s2(const float *in, const void *Ws, int B, int cin, int cout, int H, int W, int ksize,
                                float *out, void *stream);
RSLO_API int rslo_conv2d_dgrad_s2(const float *dout, const void *Ws, int B, int cin, int cout, int H, int W, int ksize,
                                  float *din, void *stream);
/*      din = data gradient + res (res [B,cin,H,W]): the input gradients of the two branches of a stride-2 BasicBlock
 *      (custom_resnet_spc.py:74-96) joined in the second branch's epilogue, same bits as the add.  ksize 1 only: res may
 *      BE din (in place) -- the 1x1 gradient lands on the pixels (2y, 2x), the other three quarters of din are not touched. */
RSLO_API int rslo_conv2d_dgrad_s2_add(const float *dout, const void *Ws, const float *res, int B, int cin, int cout, int H,
                                      int W, int ksize, float *din, void *stream);
/*      Eval-mode (running-statistics) BatchNorm folded into the epilogue of the forward convolutions (the streaming
 *      odometry path, rslo_amd/inference.py OdometryRunner):  v = (conv + bias[m]) * scale[m] + shift[m];  v += res[o]
 *      (res may be NULL);  act != 0: v = v >= 0 ? v : slope * v (slope 0 = ReLU).  rslo_conv2d_fwd_bn: 3x3, stride 1,
 *      padding 1 (Ws from rslo_conv2d_wsplit, transpose 0); rslo_conv2d_fwd_s2_bn: stride 2, ksize 3 / 1 (Ws from
 *      rslo_conv2d_wsplit_k, transpose 0).  bias, res may be NULL; res must not alias out.
 *      rslo_bn_fold_many: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale for all layers
 *      of a model in one launch (gamma / beta NULL: affine-free layer); max_c = the largest C. */
RSLO_API int rslo_conv2d_fwd_bn(const float *in, const void *Ws, const float *bias, const float *scale, const float *shift,
                                const float *res, int B, int cin, int cout, int H, int W, int act, float slope, float *out,
                                void *stream);
RSLO_API int rslo_conv2d_fwd_s2_bn(const float *in, const void *Ws, const float *bias, const float *scale,
                                   const float *shift, const float *res, int B, int cin, int cout, int H, int W, int ksize,
                                   int act, float slope, float *out, void *stream);
typedef struct {
  const float *gamma, *beta;        /* affine parameters [C] (NULL: 1 / 0) */
  const float *mean, *var;          /* running statistics [C] */
  float *scale, *shift;             /* [C] outputs */
  int32_t C;
  float eps;
} RsloBnFoldDesc;
RSLO_API int rslo_bn_fold_many(const RsloBnFoldDesc *desc_dev, int n_layers, int max_c, void *stream);
/*      Pose chaining of a streamed sequence (rslo/utils/geometric.py odom_to_abs_pose one scan at a time), one thread:
 *      n = *count; the scan's odometry (t [3], q [4] wxyz, fp32).  n == 0 seeds the float64 state with (t, q) and emits
 *      the identity; n >= 1: t_s += rotate(t, q_s), q_s = qmult(q_s, q) / (|.| + 1e-6), emits (t_s, q_s).  Row n of
 *      rel_rows [cap,7] (fp32) and traj [cap,7] (fp64) is written while n < cap; *count = n + 1. */
RSLO_API int rslo_pose_chain(const float *t, const float *q, double *state, int32_t *count, float *rel_rows, double *traj,
                             int cap, void *stream);
/*      C4 (bf16 operands, fp32 accumulation and storage): the same kernels issuing only the product of the
 *      round-to-nearest bf16 values of activations and weights (1 MFMA instead of 6).  Ws is the operand block of
 *      rslo_conv2d_wsplit (its first plane IS the bf16-rounded weight); the stride-2 weight gradient keeps the split form. */
RSLO_API int rslo_conv2d_fwd_bf16(const float *in, const void *Ws, const float *bias, int B, int cin, int cout, int H,
                                  int W, float *out, void *stream);
/*      Weight gradient of the 1x1 / stride-2 / padding-0 downsample layers (custom_resnet_spc.py:224-260 `downsample`):
 *      in [B,cin,H,W], dout [B,cout,Ho,Wo] -> dW [cout,cin,1,1]; the centre tap of the stride-2 3x3 kernel, same fixed-order
 *      slab reduction (bit-reproducible).  cin % 16 == 0, cout % 32 == 0, W >= 15. */
RSLO_API int rslo_conv1x1s2_wgrad_supported(int cin, int cout, int H, int W);
RSLO_API size_t rslo_conv1x1s2_wgrad_ws_bytes(int B, int cin, int cout, int H, int W);
RSLO_API int rslo_conv1x1s2_wgrad(const float *in, const float *dout, int B, int cin, int cout, int H, int W, float *dW,
                                  void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_conv2d_fwd_add_bf16(const float *in, const void *Ws, const float *bias, const float *res, int B,
                                      int cin, int cout, int H, int W, float *out, void *stream);
RSLO_API int rslo_conv2d_wgrad_bf16(const float *in, const float *dout, int B, int cin, int cout, int H, int W,
                                    int stride, float *dW, float *dbias, void *ws, size_t ws_bytes, void *stream);

/* a11 / a12  the 1x1 output convolutions of the head (torch.nn.Conv2d(c, 7, 1) / (32, 1, 1): rslo/models/odom_pred.py:71,
 *      rslo/models/odom_pred_base.py:22-24,107-109), cout <= 8, NCHW fp32, HW = H * W:
 *      forward (+ bias), data gradient, weight gradient (+ bias gradient from the same pass, fixed summation order). */
RSLO_API int rslo_conv1x1_supported(int cin, int cout);
RSLO_API int rslo_conv1x1_fwd(const float *x, const float *W, const float *bias, int B, int cin, int cout, int HW,
                              float *out, void *stream);
RSLO_API int rslo_conv1x1_dgrad(const float *dy, const float *W, int B, int cin, int cout, int HW, float *dx, void *stream);
RSLO_API size_t rslo_conv1x1_wgrad_ws_bytes(int B, int cin, int cout, int HW);
RSLO_API int rslo_conv1x1_wgrad(const float *x, const float *dy, int B, int cin, int cout, int HW, float *dW, float *dbias,
                                void *ws, size_t ws_bytes, void *stream);

/* a16 / a20  per-pair pose algebra of the loss assembly (one thread per frame pair):
 *      rslo_quat_to_rot: q (w,x,y,z) -> R [B,9] with kornia 0.4.0 semantics (normalise with eps 1e-12 first;
 *      rslo/models/voxel_odom_net.py:675) and its backward;  rslo_pose_targets: pseudo-targets of the ICP refinement
 *      (voxel_odom_net.py:709-735): q* = sign-fixed (w,x,y,z) quaternion of res_R R_pred (kornia's four-branch
 *      matrix -> quaternion, eps 1e-8), t* = res_R T_pred + res_t. */
RSLO_API int rslo_quat_to_rot(const float *q_wxyz, int B, float *R, void *stream);
RSLO_API int rslo_quat_to_rot_bwd(const float *q_wxyz, const float *gR, int B, float *gq, void *stream);
RSLO_API int rslo_pose_targets(const float *res_r, const float *res_t, const float *R_pred, const float *T_pred, int B,
                               float *rot_targets_wxyz, float *trans_targets, void *stream);
/*      _tq: additionally the rows (t*, q*) [B,7] the pyramid supervision reads (voxel_odom_net.py:747), NULL = skip. */
RSLO_API int rslo_pose_targets_tq(const float *res_r, const float *res_t, const float *R_pred, const float *T_pred, int B,
                                  float *rot_targets_wxyz, float *trans_targets, float *tq, void *stream);

/* f1   optimizer step of the training driver: global gradient-norm clipping (train_hdf5.py:671,
 *      torch.nn.utils.clip_grad_norm_) and torch.optim.Adam under the fastai OptimWrapper's decoupled weight decay
 *      (rslo/torchplus/train/fastai_optim.py:176-187; 8 parameter groups, rslo/builder/optimizer_builder.py:49-66) over
 *      all parameter tensors at once.  tensors_dev: device array, one entry per trainable tensor (grad = NULL: no
 *      gradient this step -- excluded from the norm, decayed but not stepped, like the wrapper does);
 *      chunks_dev: device array cutting the tensors into pieces of <= 4096 elements (offsets multiples of 4), one
 *      workgroup each.  State lives in the caller's tensors (exp_avg, exp_avg_sq, step = torch.optim.Adam's).
 *      rslo_opt_clip_grad_norm: total_norm[0] = || all grads ||_2 (device scalar, no host read); grads are scaled by
 *      max_norm / (total_norm + 1e-6) when that is < 1.  partial_ws: n_chunks doubles.
 *      rslo_opt_adam_step: p *= 1 - wd lr; m, v moment updates; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *      with t = step (the count AFTER this update, >= 1); writes t into every tensor's step scalar. */
typedef struct {
  float *param, *grad, *exp_avg, *exp_avg_sq, *step;   /* step may be NULL */
  int32_t group;                                       /* index into RsloOptHyper.group */
  int32_t step_offset;  /* this tensor's own step count = `step` + step_offset (torch.optim.Adam counts per tensor: one
                           that got its first gradient late, or skipped steps, lags the others) */
} RsloOptTensor;
typedef struct {
  int32_t tensor, count;
  int64_t offset;
} RsloOptChunk;
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;          /* weight_decay = the wrapper's decoupled wd (0: none) */
} RsloOptGroup;
#define RSLO_OPT_MAX_GROUPS 16
typedef struct {
  RsloOptGroup group[RSLO_OPT_MAX_GROUPS];
} RsloOptHyper;
RSLO_API int rslo_opt_clip_grad_norm(const RsloOptTensor *tensors_dev, const RsloOptChunk *chunks_dev, int n_chunks,
                                     float max_norm, double *partial_ws, float *total_norm, void *stream);
RSLO_API int rslo_opt_adam_step(const RsloOptTensor *tensors_dev, const RsloOptChunk *chunks_dev, int n_chunks,
                                const RsloOptHyper *hyper, float step, void *stream);

/* ---- a6 / a10 second stage (round 6): all weight-gradient reduces of a backward pass in ONE launch.
 *      Every weight-gradient entry point (rslo_conv2d_wgrad[_bf16], rslo_conv1x1s2_wgrad, rslo_spconv_wgrad_pairs[_bf16]) is a
 *      kernel that leaves slab / chunk partials in the caller's workspace + a small kernel that adds them in a fixed order.  While
 *      a sink is installed (rslo_wgrad_reduce_defer(sink, capacity, &count)) they append a descriptor of that second kernel to
 *      the caller's array instead of launching it (count is advanced; a full sink: launched at once, as without one);
 *      rslo_wgrad_reduce_defer(NULL, 0, NULL) removes the sink (the sink is per calling THREAD).  rslo_wgrad_reduce_many(reduces, n, stream) then runs the n
 *      reduces as one grid -- the same block bodies, the same bits.  The caller keeps every workspace / bias-partial buffer a
 *      descriptor points to alive and unmodified until that launch, and orders it behind the kernels that wrote them (same
 *      stream or an event).  Nothing of the reference reads a gradient before the pass is over (train_hdf5.py:663-672). */
typedef struct RsloWgradReduce {
  int32_t kind;               /* 0: dense slab partials (conv2d.hip); 2: sparse pair-chunk partials (spconv.hip) */
  int32_t n_blocks;           /* workgroups of 256 threads */
  const void *ws;
  void *dW;
  const void *aux;            /* bias-gradient partial rows */
  void *dbias;
  const void *koff;           /* sparse: pair offsets per kernel offset */
  int32_t p[8];               /* shape parameters, written by the launch code */
} RsloWgradReduce;
RSLO_API int rslo_wgrad_reduce_defer(RsloWgradReduce *sink, int capacity, int *count);
RSLO_API int rslo_wgrad_reduce_many(const RsloWgradReduce *reduces, int n, void *stream);

/* ---- a22 (SyncBN statistics): sum of a few hundred doubles over the ranks of ONE node, as a kernel on the caller's stream
 *      Replaces the per-layer all-reduce of apex SyncBatchNorm (rslo/layers/SparseConv.py:96-132 -> apex
 *      sync_batchnorm: 45 layers x 2 directions per step, train_hdf5.py:463) between rslo_bn2d_stats and rslo_bn2d_apply
 *      (and rslo_bn2d_bwd_reduce / _bwd_apply).  Every rank owns a slice (4 slots of {flag, payload}) the others can read;
 *      rslo_peer_allreduce_f64 writes the own payload + flag, waits for every peer's flag of the same exchange number, and
 *      sums the payloads in rank order (identical bits on every rank) into t, in place.  All ranks must issue the same
 *      sequence of exchanges, and all exchanges of one comm go to ONE stream (slot reuse relies on their order).  A peer that does not arrive within the timeout (default 600 s, rslo_peer_set_timeout_ms) poisons t with NaN and is
 *      reported by rslo_peer_status -- the kernel never hangs the GPU.
 *      Transports:  host   = one POSIX shared-memory segment `name` (every rank passes the same name) registered with the
 *                            HIP runtime: any GPUs of one host, also several ranks on one GPU;
 *                   device = each rank's slice in its own HBM, exported as an IPC handle of rslo_peer_ipc_handle_bytes()
 *                            bytes (begin), the handles of ALL ranks in rank order handed back (finish): peers read it
 *                            over xGMI.  world <= 16, max_n <= 1024. */
RSLO_API int rslo_peer_create_host(const char *name, int rank, int world, int max_n, void **comm_out);
RSLO_API int rslo_peer_host_unlink(void *comm);   /* after the caller's barrier: drop the segment's name (mappings stay) */
RSLO_API int rslo_peer_ipc_handle_bytes(void);
RSLO_API int rslo_peer_create_device_begin(int rank, int world, int max_n, void **comm_out, void *handle_out);
RSLO_API int rslo_peer_create_device_finish(void *comm, const void *all_handles);
RSLO_API int rslo_peer_set_timeout_ms(void *comm, int ms);
RSLO_API int rslo_peer_allreduce_f64(void *comm, double *t, int n, void *stream);
RSLO_API unsigned long long rslo_peer_status(void *comm, int *peer);
/*      Diagnostics for the first real N > 1 run: microseconds each of the most recent exchanges (<= 4096) spent spinning for its
 *      slowest peer, oldest first (arrival skew + transport latency); returns the sample count. */
RSLO_API int rslo_peer_wait_samples(void *comm, float *out_us, int max_out);
/*      Round 5: SyncBN of the maps a workgroup holds in registers (N*HW <= 17408 values per channel, C <= 512) in ONE launch
 *      per direction on any number of ranks.  The workgroup of channel c publishes its sums in the comm's slice, meets the
 *      workgroups of channel c on the other ranks (per-channel flags; sums in rank order: identical bits everywhere) and
 *      applies from its registers -- no statistics kernel, no exchange kernel, no second pass over the activation.  Same
 *      exchange sequence rule as rslo_peer_allreduce_f64 (one sequence number per call, all on one stream); a missing peer
 *      poisons the outputs with NaN and is reported by rslo_peer_status.  count_out / count_all: the element count over
 *      all ranks (device double), produced by the forward pass and read by the backward pass.  Replaces apex
 *      SyncBatchNorm forward / backward (rslo/layers/SparseConv.py:96-132) as rslo_bn2d_fwd_local / _bwd_local do on one rank. */
RSLO_API int rslo_bn2d_peer_supported(int N, int C, int HW);
RSLO_API int rslo_bn2d_fwd_peer(void *comm, const float *x, const float *res, const float *gamma, const float *beta, int N,
                                int C, int HW, float eps, float momentum, float act_slope, float *running_mean,
                                float *running_var, float *save_mean, float *save_invstd, double *count_out, float *y,
                                void *stream);
RSLO_API int rslo_bn2d_bwd_peer(void *comm, const float *dy, const float *y, const float *x, const float *gamma,
                                const float *save_mean, const float *save_invstd, const double *count_all, int N, int C,
                                int HW, float act_slope, int has_act, float *dx, float *dres, float *dgamma, float *dbeta,
                                void *stream);
/*      Round 6: exchanges inside a REPLAYED stream capture (the BEV head's forward as one hipGraph, rslo_amd/headgraph.py --
 *      the reference runs the same 45 SyncBatchNorm layers per step under apex DDP, train_hdf5.py:463).  Between
 *      rslo_peer_capture_begin and _end every exchange launched on the comm (rslo_peer_allreduce_f64, rslo_bn2d_fwd_peer /
 *      _bwd_peer) carries its number RELATIVE to a device word: its launch arguments are replay-invariant.  _end returns how
 *      many exchanges the capture holds.  In front of EVERY replay the caller issues rslo_peer_replay_prepare(comm, n, stream)
 *      on the replaying stream: it writes the word (= exchanges issued so far) in stream order and advances the comm's counter
 *      past the replay's n exchanges.  Every rank must capture the same exchanges in the same order (they run the same model). */
RSLO_API int rslo_peer_capture_begin(void *comm);
RSLO_API int rslo_peer_capture_end(void *comm, int *n_exchanges);
RSLO_API int rslo_peer_replay_prepare(void *comm, int n_exchanges, void *stream);
RSLO_API int rslo_peer_destroy(void *comm);

/* ------------------------------------------------------------------------------------
 * Point normals of a raw scan (csrc/normals.hip).  Replaces the offline step of script/create_hdf5.py:130-147:
 *     pcd.estimate_normals(KDTreeSearchParamHybrid(radius=0.6, max_nn=30)); pcd.orient_normals_towards_camera_location((0,0,0))
 * Open3D is not part of the reference tree: the rules are recalled from it, not verified against it; their float64
 * restatement is rslo_amd/normals.py.  For every point i of ONE cloud:
 *   neighbours = the points j with |p_j - p_i|^2 < radius^2 (strict, i included), at most the max_nn nearest, ties to
 *   the lower index; counts[i] = how many.  counts[i] >= 3: normals[i] = unit eigenvector of the smallest eigenvalue of
 *   the neighbours' covariance, else (0, 0, 1); flipped when it points away from the viewpoint (h_viewpoint3: three HOST
 *   floats read during the call, NULL = the origin).  zero_vertical != 0 applies the reader's rule
 *   (rslo/data/kitti_dataset_hdf5.py:197-198): a component whose absolute value equals that of (0, 0, 1) becomes 0.
 *   A point with a non-finite coordinate is nobody's neighbour: counts = 0, normal = 0.
 * points is read as points[i * stride_floats + 0..2] (stride_floats >= 3): a [P,4] scan or a [P,7] cloud needs no copy.
 * max_nn in 3..32, radius > 0.  N == 0 is a successful no-op.  counts may be NULL.  Six launches on `stream`, no host
 * read, nothing allocated: capturable.  Two calls on the same input give the same bits.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_normals_ws_bytes(int N);
RSLO_API int rslo_estimate_normals(const float *points, int stride_floats, int N, float radius, int max_nn,
                                   const float *h_viewpoint3, int zero_vertical, float *normals /*[N,3]*/,
                                   int32_t *counts /*[N]*/, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Voxel down-sample of a cloud (csrc/downsample.hip).  Replaces the second offline step of script/create_hdf5.py:149-165
 * (pcd.voxel_down_sample(size), called at :337-347 for 0.1 / 0.2 / 0.4 / 0.8 m, each from the full-resolution cloud).
 * Open3D is not part of the reference tree: the rules are recalled from its PointCloud::VoxelDownSample, not verified
 * against it; their float64 restatement is rslo_amd/downsample.py.  All arithmetic is double (Open3D holds doubles):
 *   a point is valid when its three coordinates are finite; an invalid point belongs to no voxel.
 *   minb = component-wise minimum of the valid points, vmin = minb - 0.5 * voxel_size,
 *   cell = floor((double(p) - vmin) / voxel_size) per axis, a true IEEE division.
 *   One output row per occupied cell: sum(p) / n, then (normals != NULL) sum(normal) / n, not renormalised; the sums
 *   are formed in ascending input index and the row is rounded to fp32 on store.
 * Fixed here, not by Open3D (whose order is that of an unordered_map): rows come in ascending (cx, cy, cz), cx most
 * significant.  A cell index >= 2^21 does not fit the sort key: then counts = {0, 1} and NOTHING ELSE is written.
 * points is read as points[i * stride_floats + 0..2], normals as normals[i * nstride_floats + 0..2] (both strides >= 3):
 * a [P,7] cloud is read in place with points = cloud, normals = cloud + 4, both strides 7.
 * out is [N, 6] (normals == NULL: [N, 3]); rows >= Q are untouched.  voxel_of_point [N] (may be NULL): output row of
 * point i, -1 for an invalid point.  npts [N] (may be NULL): points per output row, rows >= Q untouched.
 * counts [2] = {Q, flags} (flag bit 0: overflow).  N == 0 writes counts = {0, 0} and nothing else.  voxel_size <= 0 or
 * a stride < 3 is RSLO_EINVAL.  Everything runs on `stream`, no host read, nothing allocated: capturable.  Two calls
 * on the same input give the same bits.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_voxel_downsample_ws_bytes(int N);
RSLO_API int rslo_voxel_downsample(const float *points, int stride_floats, const float *normals /*or NULL*/,
                                   int nstride_floats, int N, double voxel_size, float *out /*[N,6] | [N,3]*/,
                                   int32_t *voxel_of_point /*[N] or NULL*/, int32_t *npts /*[N] or NULL*/,
                                   int32_t *counts /*[2]*/, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * World voxel map of a streamed trajectory (csrc/map.hip): a persistent, unbounded, incrementally filled voxel hash
 * in the frame of the trajectory (the frame of scan 0).  Nothing of the reference corresponds to it (evaluate.py:363-408
 * writes poses only); the float64 restatement of the rules is rslo_amd/mapping.py (VoxelMapRef), and the tests compare
 * bit for bit.  A map is a set of cubic cells of edge voxel_size (> 0); voxel_size, min_range and max_range
 * (0 <= min_range < max_range, max_range may be +inf) are fixed by rslo_map_reset.
 * Inserting scan number s (s = inserts since the last reset; the counter lives in the map) under pose7 = (t, q wxyz), 7
 * DEVICE doubles (a row of rslo_pose_chain's traj), does for every point i, in IEEE double without contraction:
 *   p = double(xyz_i).  A point with a non-finite coordinate, or whose d2 = p.x*p.x + p.y*p.y + p.z*p.z (left to right)
 *   fails d2 >= min_range*min_range && d2 < max_range*max_range, is skipped (dropped_invalid).
 *   w = t + (p + (2.0*b*q.w + 2.0*c)), b = v x p, c = v x b, v = (q.x, q.y, q.z), cross products as a.y*b.z - a.z*b.y, ...
 *   -- rslo_pose_chain's arithmetic and convention (w = T_abs p); q is NOT renormalised.
 *   cell = floor(w / voxel_size) per axis (a true division); a point with any |cell| >= 2^20 (or a non-finite w) is
 *   dropped (dropped_range).  key = (cell + 2^20) of x, y, z in 3 x 21 bits (x most significant); all-ones = empty.
 *   tag = (uint64(s) << 32) | i.
 * Every occupied cell holds  tag: the SMALLEST tag of all points ever inserted into it (the earliest scan wins, inside
 * a scan the lowest index);  hits: int32 count of all points ever inserted into it;  row: (float(w.x), float(w.y),
 * float(w.z), intensity) of the point that owns the tag (intensity = column 3 for width >= 4, else 0).  s only grows:
 * a cell created by an earlier scan never changes its row, later scans only raise hits.
 * Storage: ONE caller-owned device allocation of rslo_map_bytes(capacity) bytes, capacity = slots, a power of two in
 * 1024 .. 2^31:  header (256 bytes) | keys u64 [capacity] | tags u64 [capacity] | rows f32 [capacity, 4] | hits i32
 * [capacity].  The header as int64 words: [0] magic, [1] capacity, [2..4] voxel_size, min_range, max_range (doubles),
 * [RSLO_MAP_HDR_COUNTERS + 0..5] = n_scans, n_cells, n_points (accepted), dropped_invalid, dropped_range, dropped_full,
 * [RSLO_MAP_HDR_PRUNE + 0..2] = n_prunes, n_evicted, n_lost ("Rolling local map" below),
 * [RSLO_MAP_HDR_CARVE + 0..1] = n_carves, n_carved ("Free-space carving" below)
 * -- integer atomics only, so they are deterministic.  Open addressing, linear probing from a 64-bit mix of the key.
 * Probing is BOUNDED: at most RSLO_MAP_MAX_PROBE slots are examined; a point that finds neither its key nor an empty
 * slot among them is dropped (dropped_full).  No loop depends on the table having room: a full map costs a counter,
 * never a hang.  Between two prunes (below) slots only fill and keys never move, so a cell is either stored with its
 * complete, correct tag / hits / row, or ALL of its points are dropped; which cells are dropped once dropped_full > 0
 * depends on the race for slots and is unspecified, as is the slot a cell occupies (consumers sort by tag).  Everything
 * else is fully specified.
 *   rslo_map_bytes   host only; 0 for a capacity that is not a power of two in 1024 .. 2^31.
 *   rslo_map_reset   empties the table and writes the header, in one kernel.  An argument error (capacity, map_bytes <
 *                    rslo_map_bytes(capacity), voxel_size, ranges) is RSLO_EINVAL and writes nothing.
 *   The calls below take the map_bytes handed to rslo_map_reset and read the capacity from the header; on an
 *   allocation that was never reset (no magic, or a capacity the bytes cannot hold) their kernels do nothing.
 *   rslo_map_insert  points[i*stride_floats + 0..2] are read in place (a [P,4] scan or a [P,7] cloud needs no copy),
 *                    width >= 4 reads the intensity at column 3.  ws: rslo_map_insert_ws_bytes(N).  N == 0 still
 *                    counts as a scan.  At most three launches: slots / tags / hits by atomics; the rows of new cells,
 *                    written by the owner of the tag; the scan counter.  stride_floats < 3 is RSLO_EINVAL.
 *   rslo_map_lookup  read-only, same validity rules and the same bounded probe: hits_out[i] = -1 for a skipped or
 *                    out-of-range point, 0 for a cell that is not in the map, else the cell's hits; tags_out (may be
 *                    NULL) = the cell's tag, all-ones where hits_out <= 0.
 *   rslo_map_export  the cells with hits >= min_hits and, when center3 (3 device doubles) is given, with the squared
 *                    distance of row.xyz to it (in double, summed left to right) < radius*radius.  Order unspecified.
 *                    counts = {matching, written}: rows beyond max_rows are counted, not written (max_rows = 0: the
 *                    outputs may be NULL).
 *   rslo_map_insert_frames  every frame of a keyframe store ("Loop verification" below; store, store_bytes, capacity
 *                    and K as handed to rslo_keyframe_reset) under a pose of its own: the map after loop closure.
 *                    Let n = min(the store's n_entries, read on the device; n_poses).  The call leaves the map, every
 *                    header counter and n_scans included, in the state that n successive rslo_map_insert calls would
 *                    leave, call e = 0 .. n-1 inserting the first count_e rows of entry e as points (stride 4, width 4,
 *                    N = count_e) under pose7 = poses + 7*e (device doubles, [n_poses, 7]).  So with S0 = n_scans on
 *                    entry the point at row i of frame e has tag ((S0 + e) << 32) | i; an empty frame still counts as a
 *                    scan; a pose row that is not finite drops that frame's valid points into dropped_range (its w is
 *                    not finite); the map's range gate applies to keyframe points as to any other.  The equivalence is
 *                    exact: the smallest tag wins and hits and counters are integer sums, so the content does not
 *                    depend on the order of insertion.  Once dropped_full > 0 which cells are stored is unspecified,
 *                    as above; each stored cell is still exact.  Three launches whatever the data, no workspace: one
 *                    thread per (frame, row) in tiles of 256 rows, the grid sized from n_poses and K and held to 2048
 *                    workgroups, which take further tiles in a loop and add their counters to the header once (tiles
 *                    of frames >= n are not visited, threads >= count_e skip); the rows of new cells, by a pass over the
 *                    table's SLOTS (a tag with a scan number in [S0, S0 + n) names its owner, whose position is
 *                    recomputed from the store); n_scans += n.
 *                    RSLO_EINVAL, before the first launch and writing nothing: a null map, store or poses; a store
 *                    that is not 16-byte aligned; n_poses < 0; a capacity or K that rslo_keyframe_bytes refuses;
 *                    store_bytes below rslo_keyframe_bytes(capacity, K); map_bytes below rslo_map_bytes(1024).
 *                    n_poses == 0 is a success that launches nothing.  On a map that was never reset, or a store
 *                    whose header disagrees with (capacity, K), the kernels do nothing.
 * All of them: everything on `stream`, no host read, nothing allocated: capturable.
 *
 * Rolling local map (rslo_map_prune): the one call that removes cells.  S = n_scans at the time of the call.  A stored
 * cell with row (x, y, z, .), tag and hits is KEPT iff both hold:
 *   1. near:  center3 is NULL, or d2 < radius*radius with dx = double(x) - c[0], dy, dz likewise and
 *      d2 = dx*dx + dy*dy + dz*dz summed left to right, IEEE double without contraction -- the test of rslo_map_export.
 *      A comparison that is false evicts (a NaN centre coordinate, radius == 0); radius = +inf keeps every cell.
 *   2. not sparse:  hits >= min_hits, or S - 1 - (tag >> 32) < grace (the cell was created fewer than `grace` scans
 *      ago: it is still young).  min_hits >= 1, grace >= 0; with min_hits = 1 nothing is sparse.
 * Every other cell is EVICTED: its key, tag, row and hits are gone, rslo_map_lookup reads 0 for it, rslo_map_nearest
 * does not see it, and a later insert into it creates it afresh (new tag, hits counted from zero).  Kept cells keep
 * tag, row and hits to the bit.  n_cells becomes the number of kept cells; n_scans, n_points and the dropped_*
 * counters are cumulative and do not change.  Header words [RSLO_MAP_HDR_PRUNE + 0..2] = n_prunes (calls), n_evicted
 * (cumulative), n_lost (below); rslo_map_reset zeroes them.
 * The table is REBUILT, in place (`map` and its layout do not change): the kept records are staged in the caller-owned
 * workspace of rslo_map_prune_ws_bytes(capacity) bytes (36 per slot plus a control block), every slot is emptied, and
 * the records are inserted again under the same bounded probe.  A record that finds no empty slot among
 * RSLO_MAP_MAX_PROBE is dropped whole and counted in n_lost (n_cells excludes it): this cannot happen while the
 * longest run of occupied slots of the survivors, wrap-around included, is below RSLO_MAP_MAX_PROBE, whatever the
 * thread order, because the occupied set of a linear-probing table does not depend on the insertion order; beyond
 * that the surviving set is unspecified, like the stored set once dropped_full > 0.  A call that evicts nothing
 * leaves every slot as it is, to the byte, and only counts itself in n_prunes.
 *   rslo_map_prune_ws_bytes  host only; 0 for a capacity rslo_map_bytes refuses.
 *   rslo_map_prune   center3: 3 DEVICE doubles (a row of rslo_pose_chain's traj will do: its first three are t), or
 *                    NULL (rule 2 alone; the radius is then ignored).  radius < 0 or NaN with a centre,
 *                    min_hits < 1, grace < 0, a null or misaligned (16 bytes) workspace: RSLO_EINVAL; ws_bytes below
 *                    rslo_map_prune_ws_bytes of the capacity map_bytes can hold: RSLO_EWS.  Neither writes anything.
 *                    Five launches whatever the data; no host read, nothing allocated: capturable.
 * ------------------------------------------------------------------------------------ */
#define RSLO_MAP_MAX_PROBE 128
#define RSLO_MAP_HDR_COUNTERS 8
#define RSLO_MAP_HDR_PRUNE 5
RSLO_API size_t rslo_map_bytes(int64_t capacity);
RSLO_API int rslo_map_reset(void *map, size_t map_bytes, int64_t capacity, double voxel_size, double min_range,
                            double max_range, void *stream);
RSLO_API size_t rslo_map_insert_ws_bytes(int N);
RSLO_API int rslo_map_insert(void *map, size_t map_bytes, const float *points, int stride_floats, int width, int N,
                             const double *pose7, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_map_lookup(const void *map, size_t map_bytes, const float *points, int stride_floats, int N,
                             const double *pose7, int32_t *hits_out /*[N]*/, uint64_t *tags_out /*[N] or NULL*/,
                             void *stream);
RSLO_API int rslo_map_export(const void *map, size_t map_bytes, int min_hits, const double *center3 /*or NULL*/,
                             double radius, float *rows /*[max_rows,4]*/, uint64_t *tags /*[max_rows]*/,
                             int32_t *hits /*[max_rows]*/, int64_t max_rows, int64_t *counts /*[2]*/, void *stream);
RSLO_API int rslo_map_insert_frames(void *map, size_t map_bytes, const void *store, size_t store_bytes, int64_t capacity,
                                    int K, const double *poses /*[n_poses,7] device*/, int n_poses, void *stream);
RSLO_API size_t rslo_map_prune_ws_bytes(int64_t capacity);
RSLO_API int rslo_map_prune(void *map, size_t map_bytes, const double *center3 /*device, or NULL*/, double radius,
                            int min_hits, int grace, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Free-space carving (csrc/carve.hip): evict the cells of a world voxel map that the current scan sees THROUGH -- the
 * trail a moving object leaves in a map that otherwise only fills.  A visibility check in the style of Removert: a range
 * image of the scan, and one test per stored cell.  The float64 restatement is rslo_amd/carve.py (range_image_ref) and
 * rslo_amd/mapping.py (VoxelMapRef.carve); the tests compare bit for bit.  All arithmetic is IEEE double without
 * contraction, in the order written.
 * The pixel of a sensor-frame position (x, y, z) with rho2 = x*x + y*y != 0, in an image of H rows (1 .. 256) and W
 * columns (8 .. 4096) that spans the elevation tangents [tan_lo, tan_hi) (finite, tan_lo < tan_hi):
 *   col = min(W-1, int(floor(f * W))), f = the azimuth turn fraction of (x, y) from -0.5, counter-clockwise -- the
 *         function of "Scan de-skewing" (csrc/azimuth.h; rslo_amd/deskew.py sweep_fraction_ref); f can round to 1.
 *   e = z / sqrt(rho2);  u = ((e - tan_lo) / (tan_hi - tan_lo)) * H;  no pixel unless u >= 0 && u < H;
 *   row = int(floor(u)).  Rows are binned in the TANGENT of the elevation: no second arctangent.
 * rslo_range_image: for point i, (x, y, z) = double(xyz_i); a point with a non-finite coordinate, with rho2 == 0 or
 *   without a pixel is skipped; r = sqrt(rho2 + z*z).  img[row*W + col] = the minimum, as uint32, of the bit patterns of
 *   float(r) over the pixel's points (positive floats order as their bits); an empty pixel holds 0xFFFFFFFF.  A minimum
 *   does not depend on arrival order: the image is reproducible to the bit.  Two launches whatever the data (fill; one
 *   thread per point with an atomic minimum); N == 0 leaves an empty image.  RSLO_EINVAL, writing nothing: H, W or the
 *   tangents outside the above, stride_floats < 3, N < 0, a null img, null points with N > 0.
 * rslo_map_carve: S = n_scans at the time of the call, pose7 = (t, q wxyz) 7 DEVICE doubles, the pose of the scan the
 *   image was made of.  A stored cell with row (x, y, z, .) and tag is EVICTED iff every one of the following holds; a
 *   comparison that is false keeps the cell, so a NaN pose carves nothing:
 *   1. old enough:  S - 1 - (tag >> 32) >= grace;
 *   2. in view:  d = double(row.xyz) - t per axis;  p = rotate(conj(q), d), conj(q) = (w, -x, -y, -z), the rotation of
 *      the insert (q NOT renormalised);  rho2 = p.x*p.x + p.y*p.y > 0;  r_m = sqrt(rho2 + p.z*p.z) < max_range
 *      (max_range may be +inf);  p has a pixel (row, col);
 *   3. observed:  img[row*W + col] is not empty;
 *   4. seen through:  m = the minimum of the non-empty pixels of the window rows row-win_rows .. row+win_rows clipped
 *      to the image, columns col-win_cols .. col+win_cols wrapped modulo W;
 *      double(float_of(m)) - r_m > margin_abs + margin_rel * r_m.
 *   The window is what keeps the ground: at grazing incidence the range of the ground changes by metres across one
 *   pixel of elevation, and the nearer return in the row below protects the cell.
 *   Evicted cells are gone exactly as after rslo_map_prune, kept cells keep tag, row and hits to the bit, and the table
 *   is rebuilt in place by prune's own launches through the same workspace; a call that evicts nothing leaves every slot
 *   as it is, to the byte.  Header words [RSLO_MAP_HDR_CARVE + 0..1] = n_carves (calls), n_carved (cells, cumulative);
 *   rslo_map_reset zeroes them.  n_cells is recounted, n_lost is added to as in the prune, n_prunes and n_evicted do
 *   not move.  Five launches whatever the data, no host read, nothing allocated: capturable.
 *   RSLO_EINVAL, writing nothing: the H, W and tangent errors above, win_rows outside 0 .. 4, win_cols outside 0 .. 8,
 *   a negative or NaN margin, !(max_range > 0), grace < 0, a null map, img, pose7 or workspace, a workspace that is not
 *   16-byte aligned; RSLO_EWS: ws_bytes below rslo_map_carve_ws_bytes (= rslo_map_prune_ws_bytes) of the capacity
 *   map_bytes can hold.
 * ------------------------------------------------------------------------------------ */
#define RSLO_MAP_HDR_CARVE 14
RSLO_API int rslo_range_image(const float *points, int stride_floats, int N, int H, int W, double tan_lo, double tan_hi,
                              uint32_t *img /*[H*W]*/, void *stream);
RSLO_API size_t rslo_map_carve_ws_bytes(int64_t capacity);
RSLO_API int rslo_map_carve(void *map, size_t map_bytes, const uint32_t *img /*[H*W]*/, int H, int W, double tan_lo,
                            double tan_hi, const double *pose7 /*device*/, int win_rows, int win_cols, double margin_abs,
                            double margin_rel, double max_range, int grace, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Scan-to-map registration (csrc/mapreg.hip): the world voxel map as a registration target.  Read-only on the map;
 * the float64 restatement is rslo_amd/mapping.py (VoxelMapRef.nearest / normal_equations / register).  All arithmetic
 * is IEEE double without contraction, in the order written here.  Every call takes the map_bytes AND the voxel_size
 * handed to rslo_map_reset: the host checks max_dist against that voxel_size, the kernels check it against the
 * header and treat a map whose cell edge differs like a map that was never reset (no match anywhere).
 * rslo_map_params reads {voxel_size, min_range, max_range} of a map into HOST memory (it synchronises `stream`; not
 * capturable) for a caller that did not keep them.
 *
 * Nearest (rslo_map_nearest).  For point i the map's own function gives the status, the world position w and the cell
 * c, with the validity rules of rslo_map_lookup.  Candidates are the 27 cells c + {-1,0,1}^3; a neighbour with any
 * |cell| >= 2^20 is skipped.  Each candidate is found with the bounded probe of rslo_map_lookup and must have
 * hits >= min_hits.  With m = double(row.xyz) of a candidate: d = w - m, d2 = d.x*d.x + d.y*d.y + d.z*d.z (left to
 * right).  The winner has the smallest d2, ties go to the smallest tag; it is accepted only if d2 < max_dist*max_dist.
 * tags_out int64 [N]: the winner's tag, -1 without a match or for an invalid point; d2_out double [N]: -1.0 without a
 * match; rows_out float [N,4] (may be NULL): the matched row, zeros without a match.  0 < max_dist <= voxel_size,
 * anything else (NaN included) is RSLO_EINVAL: under that condition the 27 cells hold every stored row within
 * max_dist of w, so the result is the exact nearest stored point.  One launch, capturable.
 *
 * Normal equations (rslo_map_normal_eq) at pose7 for metric 0 (point) or 1 (plane).  Every matched point (the match
 * of rslo_map_nearest under the same max_dist / min_hits) adds to 28 double sums and a pair count, with d = w - m:
 *   plane term, when metric == 1 and the scan normal n_s = double(columns 4..6) has n_s.n_s >= 0.25 (summed left to
 *     right; a zeroed or NaN normal fails it): n = n_s + (2.0*b*q.w + 2.0*c), b = v x n_s, c = v x b (the rotation of
 *     the map's w, not renormalised), r = n.x*d.x + n.y*d.y + n.z*d.z, a = (n, w x n):
 *     H(i,j) += a_i*a_j, g_i += a_i*r, cost += r*r.  (n is held fixed over a step.)
 *   point term, every other matched point: J = [I | -[w]x] (3 x 6, rows J0 J1 J2):
 *     H(i,j) += J0_i*J0_j + J1_i*J1_j + J2_i*J2_j, g_i += J0_i*d.x + J1_i*d.y + J2_i*d.z, cost += d.x*d.x + d.y*d.y + d.z*d.z.
 *   metric == 1 needs width >= 7 and stride_floats >= 7, else RSLO_EINVAL.
 * out29 = the upper triangle of H row by row (21), g (6), cost, then the pair count as a double.  The reduction is
 * bit-reproducible: no floating-point atomics; inside a block of 256 points a fixed shuffle tree per wave, then the
 * waves in order; the block partials are summed in block order by a second launch.  ws: rslo_map_register_ws_bytes(N),
 * 8-byte aligned.  Two launches, capturable.
 *
 * Register (rslo_map_register): `iters` (1..32) Gauss-Newton iterations on the device, pose7 updated in place.  Per
 * iteration: the normal equations at the current pose; M = H + damping*I factored by plain row-by-row 6 x 6 Cholesky
 * (fails when a pivot is <= 0 or not finite); delta = -M^-1 g = (dt, dtheta), a world-frame increment;
 * theta = |dtheta|; dq = (1, dtheta/2) when theta < 1e-12, else (cos(theta/2), sin(theta/2)/theta * dtheta);
 * q' = (dq (x) q) / sqrt(sum of squares); t' = dt + rotate(dq, t) with rslo_pose_chain's rotate formula.
 * info double [iters, 8], row = {status, pairs, cost, |dt|, theta, 0, 0, 0}; status 0: step taken; 1: pairs <
 * min_pairs, pose untouched; 2: not positive definite (or a step that is not finite), pose untouched; 3: skipped
 * because an earlier iteration had |dt| < tol_t and theta < tol_r (the row is {3, 0, ...}).  tol_t = tol_r = 0 never
 * skips.  The "converged" flag lives in the workspace; later iterations exit early.  No host read; 2 launches per
 * iteration whatever happens (1 for N == 0), so the call is capturable.  iters outside 1..32, a negative or NaN
 * tolerance: RSLO_EINVAL; a short workspace: RSLO_EWS; an argument error writes nothing.
 *
 * Robust weight (rslo_map_normal_eq_w, rslo_map_register_w: the calls above plus robust_scale).  A matched point whose
 * term -- plane or point, chosen exactly as above -- has the cost addend e (r*r, or d.x*d.x + d.y*d.y + d.z*d.z) gets
 * the Geman-McClure weight  s2 = scale*scale, u = s2 / (s2 + e), rho = u*u,  and every one of its 28 addends is the
 * addend above multiplied by rho: rho * (a_i*a_j), rho * (a_i*r), rho * (r*r), ...  The pair count stays the
 * unweighted count of matched points, `cost` becomes the weighted cost.  scale == 0 means "no weights": the sums are
 * the bits of rslo_map_normal_eq / rslo_map_register (the same kernel).  scale < 0, NaN or inf is RSLO_EINVAL, and so
 * is a positive scale whose square is not a positive finite double (|scale| below about 1.5e-162 or above 1.3e154):
 * u would be 0/0 for e == 0, or inf/inf.  Same reduction, same order, no floating-point atomics: bit-reproducible.
 * Launch counts as above (2 per iteration, 1 for N == 0): capturable.
 *
 * Scheduled register (rslo_map_register_sched): coarse-to-fine registration over several maps of the same scans with
 * different cell edges.  maps / map_bytes / voxel_sizes are HOST arrays of n_levels (1..8) entries, stages a HOST array
 * [n_stages, 4] of rows {level, iters, max_dist, robust_scale}; all are read at enqueue time.  The stages run in order
 * on the one pose7, in place; inside a stage the rules of rslo_map_register_w hold against maps[level], including
 * 0 < max_dist <= voxel_sizes[level].  The "converged" flag is cleared at the start of every stage by the stage's
 * first launches (its first iteration does not read the flag, and rewrites it), not by a host write: a met tolerance
 * skips the rest of that stage only (status 3), the next stage runs.  info double [sum of iters, 8], rows in order of
 * execution: {status, pairs, cost, |dt|, theta, stage, level, 0} (skipped rows: {3, 0, 0, 0, 0, stage, level, 0}).
 * The sum of iters is 1..64.  RSLO_EINVAL: n_levels outside 1..8, a null array or map, map_bytes below
 * rslo_map_bytes(1024), a level that is not an integer in 0..n_levels-1, a stage with iters < 1 (or not an integer),
 * a bad max_dist or scale, more than 64 iterations, and the argument errors of rslo_map_register; RSLO_EWS: ws_bytes
 * below rslo_map_register_ws_bytes(N) (unchanged).  Every stage is checked before the first launch: an error writes
 * nothing.  No host read, nothing allocated, and the number of launches depends on the schedule alone: capturable.
 * ------------------------------------------------------------------------------------ */
RSLO_API int rslo_map_params(const void *map, size_t map_bytes, double *params3_host, void *stream);
RSLO_API int rslo_map_nearest(const void *map, size_t map_bytes, double voxel_size, const float *points,
                              int stride_floats, int N, const double *pose7, double max_dist, int min_hits,
                              int64_t *tags_out /*[N]*/, double *d2_out /*[N]*/, float *rows_out /*[N,4] or NULL*/,
                              void *stream);
RSLO_API size_t rslo_map_register_ws_bytes(int N);
RSLO_API int rslo_map_normal_eq(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                int stride_floats, int width, int N, const double *pose7, int metric, double max_dist,
                                int min_hits, double *out29, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_map_register(const void *map, size_t map_bytes, double voxel_size, const float *points,
                               int stride_floats, int width, int N, double *pose7, int iters, int metric,
                               double max_dist, int min_hits, double damping, int min_pairs, double tol_t, double tol_r,
                               double *info /*[iters,8]*/, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_map_normal_eq_w(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                  int stride_floats, int width, int N, const double *pose7, int metric, double max_dist,
                                  int min_hits, double robust_scale, double *out29, void *ws, size_t ws_bytes,
                                  void *stream);
RSLO_API int rslo_map_register_w(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                 int stride_floats, int width, int N, double *pose7, int iters, int metric,
                                 double max_dist, int min_hits, double damping, int min_pairs, double tol_t, double tol_r,
                                 double robust_scale, double *info /*[iters,8]*/, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_map_register_sched(const void *const *maps /*[n_levels] host*/, const size_t *map_bytes /*host*/,
                                     const double *voxel_sizes /*host*/, int n_levels,
                                     const double *stages /*[n_stages,4] host*/, int n_stages, const float *points,
                                     int stride_floats, int width, int N, double *pose7, int metric, int min_hits,
                                     double damping, int min_pairs, double tol_t, double tol_r,
                                     double *info /*[sum of iters,8]*/, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Place recognition (csrc/places.hip): a Scan Context descriptor per scan (Kim & Kim, "Scan Context: Egocentric Spatial
 * Descriptor for Place Recognition within 3D Point Cloud Map", IROS 2018), a device-resident database of descriptors
 * and a two-stage search for the stored scans that look like a query.  The rules are recalled from the paper and fixed
 * here; rslo_amd/places.py (ScanContextRef, PlaceDBRef) restates them in float64 numpy and the tests compare bit for
 * bit.  All arithmetic is IEEE double with contraction off unless a rule says float.  No transcendental function
 * decides a bin: device and host math libraries do not agree to the bit.
 *
 * Parameters: R rings (1..64), S sectors (3..128), max_range > 0, z_offset (float).
 * Tables, made ONCE by the caller and handed to the device and to the restatement alike: `tables` is
 * 2*(S+1) + (R+1) doubles = dirs[k] = (cos(2 pi k / S), sin(2 pi k / S)) for k = 0..S with dirs[S] = dirs[0], followed
 * by edge2[k] = (k * max_range / R)^2 for k = 0..R.
 *
 * Descriptor D, float32 [R, S], of one scan in the sensor frame.  For every point i:
 *   1. x, y = double(p.x), double(p.y);
 *   2. a coordinate of xyz that is not finite drops the point (dropped_invalid);
 *   3. r2 = x*x + y*y; the point is dropped (dropped_range) unless r2 > 0 and r2 < edge2[R];
 *   4. ring = the number of k in 1..R-1 with r2 >= edge2[k];
 *   5. c_k = dirs[k].x*y - dirs[k].y*x; sector = the smallest k in 0..S-1 with c_k >= 0 and c_{k+1} < 0; none: dropped
 *      (dropped_range).  The kernel guesses k from atan2f and confirms both conditions on the same computed c values
 *      (also for the guess's two neighbours); a guess that is not confirmed falls back to the scan over k;
 *   6. v = p.z + z_offset in float; the point is dropped (dropped_low) unless v > 0;
 *   7. D[ring, sector] = max(D[ring, sector], v).  Empty bins are 0.  n_points counts the points that arrive here.
 * With it go key[r] (int32) = the number of sectors of ring r with D > 0, and norm[j] (double) = sqrt of the sum over r
 * ascending of double(D[r,j])^2.  counters4 = {n_points, dropped_invalid, dropped_range, dropped_low}, int64.
 * Positive floats order as their bit patterns: the maximum is an integer maximum (per workgroup in LDS, then into the
 * zeroed grid), which does not depend on arrival order.  Three launches (two for N == 0: an all-zero grid).
 *
 * Database: ONE caller-owned device allocation of rslo_place_bytes(capacity, R, S) bytes,
 *   header (256 bytes) | D f32 [N, R, S] | norm f64 [N, S] | key i32 [N, R],   N = capacity, sections padded to 256 bytes.
 * Header int64 words: [0] magic, [1] capacity, [2] R, [3] S, [4] n_entries, [5] dropped_full.  capacity (1 .. 2^24), R
 * and S are fixed by rslo_place_reset; add and query take them again and do nothing on an allocation whose header
 * says otherwise (never reset, or reset with other values).  rslo_place_add appends (D, key, norm) as entry number
 * n_entries (read on the device); on a full database the entry is not stored and dropped_full counts it.  Two launches.
 *
 * Query with (D, key, norm) of a scan, exclude_recent >= 0, num_candidates C in 0..256, top_k in 1..16:
 *   eligible: the entries with index < n_entries - exclude_recent;
 *   stage 1 (C > 0): kd = min(sum over r of (key_q[r] - key_e[r])^2, 2^32 - 1), the sum exact for any int32 keys (a
 *     term of |difference| >= 2^16 alone reaches the bound; nothing wraps); the C eligible entries with the smallest
 *     kd go on, ties to the lower index (composite key kd << 32 | index).  C == 0: every eligible entry goes on;
 *   stage 2: for every shift s in 0..S-1, with j' = (j + s) % S: column j is valid when norm_q[j] > 0 and
 *     norm_e[j'] > 0; dot_j = sum over r ascending of double(Dq[r,j]) * double(De[r,j']);
 *     cos_j = dot_j / (norm_q[j] * norm_e[j']); d(s) = 1 - (sum of cos_j over the valid j, ascending) / n_valid, +inf
 *     without a valid column.  The entry's distance is the smallest d(s), ties to the lowest s;
 *   result: out double [top_k, 4], rows (entry index, distance, shift, (shift * 2 pi) / S) ordered by distance, then by
 *     index; entries at +inf are not returned; unused rows are (-1, +inf, -1, 0).  Column 3 is the query's heading
 *     relative to the entry.  No threshold is applied: acceptance is the caller's comparison.
 * The S x S column dots are formed in double on the vector ALU, one workgroup per stage-2 entry; one thread per shift
 * adds its wrapped diagonal in j order.  Selection compares integers (the ordered bit pattern of the distance, then
 * the index).  Launches: 4 with C > 0, 2 with C == 0 (a grid of `capacity` workgroups); no flag between workgroups,
 * no floating-point atomic, no host read, nothing allocated: capturable.
 *
 * Errors: RSLO_EINVAL (nothing is written) for R, S, capacity or a count outside its range, a null pointer, N < 0,
 * stride_floats < 3, a z_offset that is not finite, db_bytes below rslo_place_bytes(capacity, R, S), a workspace that is
 * null or not 8-byte aligned; RSLO_EWS for ws_bytes below rslo_place_query_ws_bytes(capacity).
 * rslo_place_bytes / rslo_place_query_ws_bytes are host only and return 0 for arguments out of range.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_place_bytes(int64_t capacity, int R, int S);
RSLO_API int rslo_place_reset(void *db, size_t db_bytes, int64_t capacity, int R, int S, void *stream);
RSLO_API int rslo_place_describe(const float *points, int stride_floats, int N, int R, int S,
                                 const double *tables /*[2*(S+1) + R+1]*/, float z_offset, float *D /*[R,S]*/,
                                 int32_t *key /*[R]*/, double *norm /*[S]*/, int64_t *counters4, void *stream);
RSLO_API int rslo_place_add(void *db, size_t db_bytes, int64_t capacity, int R, int S, const float *D,
                            const int32_t *key, const double *norm, void *stream);
RSLO_API size_t rslo_place_query_ws_bytes(int64_t capacity);
RSLO_API int rslo_place_query(const void *db, size_t db_bytes, int64_t capacity, int R, int S, const float *Dq,
                              const int32_t *keyq, const double *normq, int64_t exclude_recent, int num_candidates,
                              int top_k, double *out /*[top_k,4]*/, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Pose graph (csrc/posegraph.hip): Gauss-Newton over a trajectory with loop edges, so that "scan j is at this pose
 * relative to scan i" spreads its correction over the poses in between.  The float64 restatement is
 * rslo_amd/posegraph.py (PoseGraphRef); the tests compare within rounding bounds, not bit for bit (device and host
 * sum in different orders).  All arithmetic is IEEE double with contraction off.  How a loop measurement is made, and
 * whether it is true, is the caller's business.
 *
 * Poses are [7] double rows (t, q wxyz), the trajectory's format.  compose(A, B) = (t_A + rotate(q_A, t_B), q_A (x) q_B),
 * inverse of a unit pose = (-rotate(q*, t), q*), rotate and (x) by rslo_pose_chain's formulas; products are not
 * renormalised.  rslo_pose_between writes out[k] = A[k]^-1 o B[k].
 *
 * Nodes: N (2 .. 65536).  traj0 [N,7] is the input trajectory, read only; poses [N,7] is the estimate, updated in place
 * (a copy of traj0 on a first call).  Node 0 is fixed.  Vectors over the nodes are [N,6] rows (rho, phi) with row 0
 * read as zero and written zero.
 * Chain edge k (0 .. N-2) joins node k to node k+1 with Z_k = traj0[k]^-1 o traj0[k+1], computed from traj0, and weights
 * (w_t, w_r): chain_w2_host, 2 HOST doubles, positive and finite, for the whole chain, or chain_w_dev, a DEVICE
 * [N-1,2] array that wins when it is not NULL (an entry that is not positive and finite makes its edge singular).
 * Loop edge l (L of them, 0 .. 4096): loops_ij int32 [L,2], loops_Z double [L,7] (the pose of j in the frame of i, its
 * quaternion divided by its norm on read), loops_w double [L,2].  A row is skipped and counted when i < 0 (the unused
 * row of rslo_place_query), j < 0, i or j >= N, i == j, a value of Z or w is not finite, the quaternion is zero or a
 * weight is negative.  No edge is read on the host.
 *
 * Residual of an edge (i, j, Z): A = T_i^-1 o T_j, E = Z^-1 o A, s = +1 if q_E.w >= 0 else -1,
 *   r = (w_t t_E, w_r 2 s vec(q_E)).
 * Local parametrisation T' = T o (rho, phi): t' = t + rotate(q, rho), q' = (q (x) dq(phi)) / |.| with
 * rslo_map_register's dq, its theta < 1e-12 branch included.
 * Jacobians, G = s (q_E.w I + [vec q_E]x): d r_t/d rho_j = R_E, d r_r/d phi_j = G, d r_t/d rho_i = -R_Z^T,
 * d r_t/d phi_i = R_Z^T [t_A]x, d r_r/d phi_i = -G R_A^T, all other blocks zero, rows scaled by the weights.  R(q) is
 * the matrix of the unit-quaternion formula.
 * Robust weight, loop edges only: e = r.r, s2 = scale*scale, u = s2 / (s2 + e), rho = u*u; H += rho J^T J,
 * g += rho J^T r, cost += rho e; scale == 0: rho = 1; a bad scale is refused by rslo_map_register_w's rule.  Chain
 * edges are never down-weighted, so the preconditioner stays exact.
 *
 * One Gauss-Newton iteration: linearise at poses; H = H_chain + H_loops + damping I over nodes 1 .. N-1; solve
 * H x = -g by conjugate gradients preconditioned with M = H_chain = J_c^T J_c, at most cg_iters (1 .. 256) iterations,
 * stopping when r.z <= cg_tol^2 (r.z)_0; update every pose.  J_c is block lower-bidiagonal with A_k = W dr/d delta_k
 * and B_k = W dr/d delta_{k+1} = diag(w_t R_E, w_r G), whose inverse is closed form
 * (G^-1 = (w w I - w [v]x + v v^T) / (s w (w w + v.v)) for q_E = (w, v)).  M^-1 r: backward
 * y_{m-1} = B_{m-1}^-T (r_m - A_m^T y_m), then forward z_{k+1} = B_k^-1 (y_k - A_k z_k).
 * CG stops WITHOUT applying the iteration when p.Ap is not a positive finite number; x so far is the step.  A step that
 * is entirely zero for that reason, a step that is not finite, and a singular B_k (q_E.w == 0 on a chain edge) give
 * status 2 and leave the poses untouched.  g == 0 (no usable loop on a first call, or a stationary point) is a zero
 * step with status 0 and 0 CG iterations.
 * info double [gn_iters, 8], row = {status, loops used, cost at the linearisation point, CG iterations run,
 * sqrt(r.z / (r.z)_0) at the stop, max_k |rho_k|, max_k |phi_k|, loops skipped}.  status 0: step taken; 2: failed as
 * above; 3: skipped because an earlier iteration had max|rho| < tol_t and max|phi| < tol_r (the row is {3, 0, ...});
 * the flag lives in the workspace, as in rslo_map_register.
 *
 * Kernels.  Per Gauss-Newton iteration three launches: (1) parallel over all edges: one record of
 * RSLO_PG_EDGE_DOUBLES doubles per edge, chain edges first, then loops: r[6], rho, flag (1 used, 0 skipped, 2 singular
 * chain edge), the 3 x 3 blocks A_tt, A_tr, A_rr, B_tt, B_rr row-major (A = [[A_tt, A_tr], [0, A_rr]] acts on node i,
 * B = diag(B_tt, B_rr) on node j), the gradient parts rho A^T r and rho B^T r, e, and for a chain edge B^-1's two
 * blocks; (2) ONE workgroup of 1024 threads: the gradient per node, then the whole preconditioned CG with its loop and
 * early stop inside the kernel; (3) parallel over the nodes: the update.  Sums into a node come in a fixed order, chain
 * edge n-1, chain edge n, then the loops at that node by ascending index; dot products are one fixed tree; no
 * floating-point atomic: a second call gives the same bits.  The order costs one workgroup barrier per "round": a loop
 * is added in the round of its rank among the used loops at the same node, so every H x and every gradient sum runs
 * 1 + (the largest number of used loops that share one node other than node 0) rounds.  Loops spread over the
 * trajectory cost one or two; L loops onto one node cost L rounds per CG iteration, up to 4096 x cg_iters x gn_iters
 * barriers in one call -- slow, not wrong.  The fixed node 0 receives no sum and counts no round.  The chain recurrences are scanned: each thread owns a
 * contiguous segment of ceil((N-1) / 1024) edges, runs it with zero input, a scan over the segment summaries with the
 * segments' transfer matrices (made once per Gauss-Newton iteration) gives every segment's input, and a second local
 * pass runs it with that input: dependent depth 2 * segment + log2(segments).
 * No host read, nothing allocated, 3 * gn_iters launches whatever happens: capturable.
 *
 *   rslo_posegraph_ws_bytes   host only; 0 for N or L out of range.
 *   rslo_posegraph_optimize   gn_iters 1 .. 32.
 *   rslo_posegraph_cost       out4 = {cost, chain part, loops used, loops skipped}.  Two launches.
 *   rslo_posegraph_linearize  leaves the linearisation at `poses` in the workspace; edges_out (may be NULL)
 *                             [(N-1+L), RSLO_PG_EDGE_DOUBLES], g_out (may be NULL) [N,6], sums4 as out4 above.
 *   rslo_posegraph_matvec     y = H x, rslo_posegraph_chain_solve  z = M^-1 r, both [N,6], on the linearisation a
 *                             rslo_posegraph_linearize call with the same N, L and workspace left behind (they write
 *                             nothing when the workspace holds none: rslo_posegraph_cost, rslo_posegraph_optimize
 *                             whose last linearisation had a singular chain edge, and a linearize of such a chain
 *                             clear the mark, because the scan's matrices are not made); one launch of one
 *                             workgroup each, the device functions of the solve.
 * Errors are found before the first launch and write nothing: RSLO_EINVAL for a size, count or tolerance out of
 * range (NaN included), a null pointer, a host chain weight that is not positive and finite, a bad robust_scale, a
 * workspace that is null or not 8-byte aligned, x aliasing y; RSLO_EWS for ws_bytes below rslo_posegraph_ws_bytes(N, L).
 * ------------------------------------------------------------------------------------ */
#define RSLO_PG_EDGE_DOUBLES 84
RSLO_API size_t rslo_posegraph_ws_bytes(int N, int L);
RSLO_API int rslo_posegraph_optimize(const double *traj0, double *poses, int N, const double *chain_w2_host,
                                     const double *chain_w_dev /*[N-1,2] or NULL*/, const int32_t *loops_ij,
                                     const double *loops_Z, const double *loops_w, int L, int gn_iters, int cg_iters,
                                     double cg_tol, double robust_scale, double damping, double tol_t, double tol_r,
                                     double *info /*[gn_iters,8]*/, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_posegraph_cost(const double *traj0, const double *poses, int N, const double *chain_w2_host,
                                 const double *chain_w_dev, const int32_t *loops_ij, const double *loops_Z,
                                 const double *loops_w, int L, double robust_scale, double *out4, void *ws,
                                 size_t ws_bytes, void *stream);
RSLO_API int rslo_posegraph_linearize(const double *traj0, const double *poses, int N, const double *chain_w2_host,
                                      const double *chain_w_dev, const int32_t *loops_ij, const double *loops_Z,
                                      const double *loops_w, int L, double robust_scale, double *edges_out,
                                      double *g_out, double *sums4, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_posegraph_matvec(const double *x, double *y, int N, int L, double damping, void *ws, size_t ws_bytes,
                                   void *stream);
RSLO_API int rslo_posegraph_chain_solve(const double *r, double *z, int N, int L, void *ws, size_t ws_bytes,
                                        void *stream);
RSLO_API int rslo_pose_between(const double *A, const double *B, int n, double *out /*[n,7]*/, void *stream);

/* ------------------------------------------------------------------------------------
 * Loop verification (csrc/loopverify.hip): a device-resident store of down-sampled keyframes, a geometric check that
 * turns the candidate rows of rslo_place_query into measured loop edges in ONE launch, and a device edge list that
 * rslo_posegraph_optimize reads as it is.  The float64 restatement is rslo_amd/loops.py (KeyframeStoreRef,
 * LoopVerifierRef): the store is compared bit for bit, the matching exactly, the sums within rounding bounds (device
 * and host sum in different orders).  All arithmetic is IEEE double with contraction off; the pose algebra is that of
 * the pose graph (csrc/se3.h, rslo_amd/se3.py).
 *
 * Keyframe store: ONE caller-owned device allocation (16-byte aligned) of rslo_keyframe_bytes(capacity, K) bytes,
 *   header (256 bytes) | counts i32 [capacity] | rows f32 [capacity, K, 4],   sections padded to 256 bytes.
 * Header int64 words: [0] magic, [1] capacity, [2] K, [3] 0, [4] n_entries, [5] dropped_full.  capacity is in 1 .. 2^16,
 * K a multiple of 64 in 64 .. 4096; both are fixed by rslo_keyframe_reset, and add / verify / emit take them again and
 * do nothing on an allocation whose header says otherwise.
 *
 * rslo_keyframe_prepare builds the frame [K, 4] and frame_info int32 [4] = {count, Q, flags, gated} of one scan
 * (points[i * stride_floats + 0..2], sensor frame):
 *   1. gate: a point is gated out (counted in `gated`) when a coordinate is not finite, when double(z) > min_z is
 *      false, or when x*x + y*y + z*z < max_range*max_range is false (doubles, summed left to right).  The kept points
 *      go into a [N, 3] copy in the workspace, the gated ones as NaN rows;
 *   2. rslo_voxel_downsample (its rules, no normals) at voxel_size on that copy: Q centroid rows in its cell order.
 *      Its overflow flag is flags bit 0, and then Q = count = 0;
 *   3. count = min(Q, K); frame row k = down-sample row (k * Q) / K (int64, truncating) when Q > K, else row k; column
 *      3 is 0; rows >= count are zero.
 * rslo_keyframe_add appends (frame, count) as entry n_entries (read on the device); a full store drops it and counts
 * dropped_full.  Two launches.  prepare: the down-sample's launches and three more (one for N == 0).
 *
 * rslo_loop_verify: the grid is top_k workgroups; workgroup b verifies candidate row b = (entry, distance, shift,
 * heading) of cands [top_k, 4] against the staged query frame on its own.  out double [top_k, 16], row =
 *   {status, entry, pairs of the last iteration, overlap, rms, query count, Z (7), distance, heading, 0}.
 *   status 1 (no candidate): entry >= 0 and entry < n_entries is false;
 *   status 2 (gated): distance < max_distance is false;
 *   status 3 (too few points): the query's count or the entry's count is below min_pairs.
 *   In these three cases the row is {status, entry as given, 0, 0, 0, 0, identity, 0, 0, 0}, the info rows are
 *   {status, 0 ...} and matches are -1.
 * Z is the pose of the query in the frame of the entry, p_e = Z p_q: the Z of a pose-graph loop edge (i = entry,
 * j = query).  Start: row b of `start` [top_k, 7] when it is not NULL, else t = 0, q = (cos(h/2), 0, 0, sin(h/2)) with
 * h = heading.  Match of source point i (< query count): w = rotate(q, p_i) + t; for every target point j (< the
 * entry's count) m = double(row.xyz), d = w - m, d2 = d.x*d.x + d.y*d.y + d.z*d.z; the match is the j with the smallest
 * d2, ties to the lowest j (a d2 that is NaN or +inf is never chosen), accepted iff d2 < max_dist*max_dist: the EXACT
 * nearest point within max_dist.  stages [n_stages, 2] HOST doubles {max_dist, iters}, read at enqueue: 1 .. 8 stages,
 * the iterations sum to 1 .. 64.  One iteration: every matched point adds the point term of "Scan-to-map
 * registration" (J = [I | -[w]x], residual d) to the 28 sums and the pair count; fewer than min_pairs pairs, a
 * H + damping I that is not positive definite (row-by-row Cholesky) or a step that is not finite is status 4: Z stays
 * the last good pose, the remaining iterations are skipped (their info rows are {4, 0, 0, 0, 0, stage, 0, 0}), no
 * fitness is taken (overlap = rms = 0, matches -1).  Otherwise the step is rslo_map_register's, update formulas
 * included.  info double [top_k, sum of iters, 8] (may be NULL), row = {0 or 4, pairs, cost, |dt|, theta, stage, 0, 0}.
 * Fitness at the final Z: match again with inlier_dist as the gate; overlap = inliers / query count;
 * rms = sqrt((sum of d2 over the inliers) / inliers); matches int32 [top_k, K] (may be NULL) = the matched target index
 * or -1 (also for i >= query count).  Status 0 (accepted) iff inliers > 0, overlap >= min_overlap and rms <= max_rms,
 * else 5 (without an inlier overlap = rms = 0).
 * Kernel: one workgroup of min(K, 1024) threads per candidate; the entry's frame is staged once into LDS as three
 * float planes (12 K bytes) and every source point scans all of it in ascending j, replacing on a strict `<`: exact by
 * construction.  The whole schedule and the fitness pass run inside the launch on a pose kept in LDS.  Sums: a thread's
 * own points (i = thread, thread + threads, ...) in ascending order, a shuffle tree inside each wave, the waves in
 * wave order; no floating-point atomic: two calls on the same input give the same bits, and a schedule gives the bits
 * of its iterations issued as successive single-iteration calls chained through `start`.
 *
 * Edge list: ij int32 [E, 2], Z double [E, 7], w double [E, 2], counters int64 [2] = {n_edges, dropped_full}, E in
 * 1 .. 4096.  rslo_loop_edges_reset writes i = j = -1, Z = identity, w = 0 into every row and zeroes the counters: rows
 * rslo_posegraph_optimize skips and counts, so the whole list can be handed to it without a host read.
 * rslo_loop_emit (one thread): among the rows of out [top_k, 16] with status 0 the one with the largest overlap wins,
 * ties to the lowest row; it is appended as (i = entry, j = the store's n_entries now, Z, (w_t, w_r)), or counted in
 * dropped_full when the list is full.  It runs BEFORE rslo_keyframe_add of the same scan.  At most one edge per call.
 *
 * Nothing here reads on the host (the stages excepted, at enqueue) or allocates: capturable.  Errors are found before
 * the first launch and write nothing: RSLO_EINVAL for a size, count or threshold out of range (NaN included), a null
 * or misaligned pointer, store_bytes below rslo_keyframe_bytes; RSLO_EWS for a prepare workspace (256-byte aligned)
 * below rslo_keyframe_prepare_ws_bytes(N).  rslo_keyframe_bytes returns 0 for arguments out of range.
 * ------------------------------------------------------------------------------------ */
RSLO_API size_t rslo_keyframe_bytes(int64_t capacity, int K);
RSLO_API int rslo_keyframe_reset(void *store, size_t store_bytes, int64_t capacity, int K, void *stream);
RSLO_API size_t rslo_keyframe_prepare_ws_bytes(int N);
RSLO_API int rslo_keyframe_prepare(const float *points, int stride_floats, int N, int K, double voxel_size, double min_z,
                                   double max_range, float *frame /*[K,4]*/, int32_t *frame_info /*[4]*/, void *ws,
                                   size_t ws_bytes, void *stream);
RSLO_API int rslo_keyframe_add(void *store, size_t store_bytes, int64_t capacity, int K, const float *frame,
                               const int32_t *frame_info, void *stream);
RSLO_API int rslo_loop_verify(const void *store, size_t store_bytes, int64_t capacity, int K, const float *frame,
                              const int32_t *frame_info, const double *cands /*[top_k,4]*/, int top_k,
                              const double *start /*[top_k,7] or NULL*/, const double *stages /*[n_stages,2] host*/,
                              int n_stages, double max_distance, double inlier_dist, double min_overlap, double max_rms,
                              int min_pairs, double damping, double *out /*[top_k,16]*/,
                              double *info /*[top_k,sum of iters,8] or NULL*/, int32_t *matches /*[top_k,K] or NULL*/,
                              void *stream);
RSLO_API int rslo_loop_edges_reset(int32_t *ij, double *Z, double *w, int64_t *counters2, int max_edges, void *stream);
RSLO_API int rslo_loop_emit(const double *out /*[top_k,16]*/, int top_k, const void *store, size_t store_bytes,
                            int64_t capacity, int K, int32_t *ij, double *Z, double *w, int64_t *counters2, int max_edges,
                            double w_t, double w_r, void *stream);

/* ------------------------------------------------------------------------------------
 * Surfel map (csrc/surfel.hip): a voxel hash whose cells hold the integer moments of every point inserted into them and
 * the plane those moments give, and point-to-plane registration against it that reads no scan normal.  The float64
 * restatement is rslo_amd/surfels.py SurfelMapRef: keys, moments and rows are compared BIT FOR BIT.  All arithmetic is
 * IEEE double with contraction off, in the order written; `/` and sqrt are correctly rounded.
 *
 * Storage: ONE caller-owned device allocation (8-byte aligned) of rslo_surfel_bytes(capacity) bytes,
 *   header (256 bytes) | keys u64 [cap] | moments i64 [cap, 10] | rows f64 [cap, 8] | dirty i32 [cap].
 * Header int64 words: [0] magic, [1] capacity, [2] voxel_size, [3] min_range, [4] max_range (doubles), [5] min_points
 * (>= 3), [6] planar_ratio, [7] line_ratio (doubles, >= 0, finite), [8..14] n_scans, n_cells, n_points, dropped_invalid,
 * dropped_range, dropped_full, n_planar, [RSLO_SURFEL_HDR_PRUNE + 0..2] n_prunes, n_evicted, n_lost ("Rolling local surfel
 * map" below).  The table is the world voxel map's: capacity a power of two in 1024 .. 2^31,
 * linear probing from map_mix(key), at most RSLO_MAP_MAX_PROBE slots examined; a point that finds neither its key nor an
 * empty slot is dropped and counted (dropped_full): a full table never hangs.  The ten moments of a slot are contiguous.
 * Between two prunes (below) the table only fills; rslo_surfel_reset empties it.
 *
 * Insert of a scan under pose7.
 *   1. status, world position w and key of a point are those of "World voxel map" (the same function): validity, range
 *      gate, rotation, division, |cell| < 2^20; a dropped point counts in dropped_invalid / dropped_range.
 *   2. per axis: s = w / voxel, c = floor(s), f = s - c, q = (int64) floor(f * 16384.0), clamped to 0 .. 16383 (a tiny
 *      negative s gives f == 1.0: the clamp is part of the rule).
 *   3. the cell's moments grow by (1, qx, qy, qz, qx*qx, qx*qy, qx*qz, qy*qy, qy*qz, qz*qz): 64-bit INTEGER atomics only,
 *      so the moments of a cell do not depend on the order in which points or scans arrive.
 *   4. the sums stay exact in int64 below 2^35 points per cell and convert exactly to double below 2^25.
 *   5. the slot's dirty word is set; the slot of every point is kept in the workspace (4 bytes per point).
 * Then the rows of the dirty slots are derived, and n_scans grows by one (also for N == 0).
 *
 * Derive.  The row of a cell is a pure function of its moments (N, S_a, S_ab), its key and the header.  n = double(N);
 * mu_a = double(S_a) / n; c_ab = double(S_ab) / n - mu_a * mu_b in the order 00 01 02 11 12 22; tr = (c00 + c11) + c22.
 * N < min_points or !(tr > 0 && tr < inf): the row is eight zeros (flag 0).  Otherwise a_ab = c_ab / tr; six cyclic
 * sweeps (0,1), (0,2), (1,2) of the Jacobi rotation of "Point normals" (nm_rot of csrc/normals.hip) in double, with
 * the same formulas and the same a_pq == 0 exit; l0 is the smallest diagonal entry by k_nm_normals' comparisons (ties to
 * the lower index), l1 <= l2 the other two (of the two remaining indices p < q: l1 = a_qq when a_qq < a_pp, else a_pp).
 * normal = the column e of l0 divided by sqrt((ex*ex + ey*ey) + ez*ez), negated when its component of largest magnitude
 * (ties to the lower axis) is negative.  mean_a = (double(cell_a) + (mu_a + 0.5) / 16384.0) * voxel;
 * sigma2 = ((l0 * tr) * u) * u with u = voxel / 16384.0; flag = 2.0 (planar) when l0 <= planar_ratio * l1 &&
 * l1 >= line_ratio * l2, else 1.0.  row = {mean.x, mean.y, mean.z, n.x, n.y, n.z, sigma2, flag}.  n_planar is the number
 * of rows with flag 2.0.
 *
 * rslo_surfel_insert: three launches (moments; derive, one thread per point of the scan, the thread that takes a slot's
 * dirty word derives it; the scan counter), one for N == 0.  rslo_surfel_insert_frames has the contract of
 * rslo_map_insert_frames: it leaves the table and every counter as n successive inserts of the store's frames would --
 * exactly, because everything is an integer sum and rows are functions of the sums; three launches whatever the data,
 * the derive pass running over the table's slots.  rslo_surfel_export compacts the cells with flag >= min_flag (0, 1 or
 * 2) -- and, with center3, whose mean lies within radius, by the test of rslo_map_export -- through one cursor: keys,
 * moments [R, 10] and rows [R, 8] in unspecified order, counts[2] = {matching, written}.
 *
 * Nearest (rslo_surfel_nearest).  For a point with status 0 the candidates are the cells c + {-1,0,1}^3 (neighbours
 * with |cell| >= 2^20 skipped) whose flag is 2.0, each found by the bounded probe.  d = w - mean,
 * d2 = d.x*d.x + d.y*d.y + d.z*d.z; the smallest d2 wins, then the smallest key; accepted iff d2 < max_dist*max_dist.
 * keys_out int64 [N] (-1: none), d2_out double [N] (-1.0), rows_out double [N, 8] or NULL (zeros).
 * Normal equations (rslo_surfel_normal_eq): a matched point adds the plane term of "Scan-to-map registration" with
 * n = the row's normal (world frame, not rotated), r = n.x*d.x + n.y*d.y + n.z*d.z, a = (n, w x n).  No point-term
 * fallback, no scan normal, no column beyond xyz is read.  robust_scale: the weight of "Robust weight" on e = r*r; 0
 * means no weights.  out29 and the reduction are those of rslo_map_normal_eq; no floating-point atomic.
 * Register (rslo_surfel_register): the rules of rslo_map_register_w with the normal equations above: the step, damping,
 * min_pairs, tol_t / tol_r, statuses 0..3, info rows [iters, 8], 2 launches per iteration and 1 for N == 0.
 *
 * Distribution cost (rslo_surfel_nearest_d, rslo_surfel_normal_eq_d, rslo_surfel_register_d): the point-to-distribution
 * (NDT) form.  The matched cell's covariance -- already in the table as integers -- weighs the whole residual
 * d = w - mean, so the fitted cells that fail the planar test (poles, trunks, kerbs, vegetation) take part.
 *   Candidates: the cells c + {-1,0,1}^3 whose row flag is >= min_flag, min_flag in {1, 2}.  The winner is chosen as in
 *   "Nearest" (smallest d2 to the row's mean, then smallest key) and accepted iff d2 < max_dist*max_dist.  With
 *   min_flag = 2 keys and d2 are those of rslo_surfel_nearest.
 *   Information matrix of the matched slot from its ten moments (N, S_a, S_ab): n = double(N); mu_a = double(S_a) / n;
 *   c_ab = double(S_ab) / n - mu_a * mu_b in the order 00 01 02 11 12 22 (the expressions of "Derive");
 *   u = voxel / 16384.0; C_ab = (c_ab * u) * u; lam = reg_rel * ((C00 + C11) + C22) + reg_abs * reg_abs;
 *   S = C + lam I (S_aa = C_aa + lam, the off-diagonal entries are C's);
 *     A00 = S11*S22 - S12*S12    A01 = S02*S12 - S01*S22    A02 = S01*S12 - S02*S11
 *     A11 = S00*S22 - S02*S02    A12 = S01*S02 - S00*S12    A22 = S00*S11 - S01*S01
 *   det = (S00*A00 + S01*A01) + S02*A02; M_ab = A_ab / det.  The grid is axis-aligned: M is in the world frame.
 *   reg_rel and reg_abs are >= 0, finite and not both zero.
 *   Unusable pair: a pair whose det fails det > 0 && det < inf adds nothing and is not counted.
 *   Term of a used pair, with J = [I | -[w]x] (the rows of the point term of "Scan-to-map registration") and d = w - mean:
 *     m_a = M_a0*d0 + M_a1*d1 + M_a2*d2;  e = d0*m0 + d1*m1 + d2*m2;
 *     B[a][k] = M_a0*J[0][k] + M_a1*J[1][k] + M_a2*J[2][k];
 *     H(k, l) += J[0][k]*B[0][l] + J[1][k]*B[1][l] + J[2][k]*B[2][l] for k <= l;
 *     g_k += J[0][k]*m0 + J[1][k]*m1 + J[2][k]*m2;  cost += e.
 *   The residual is dimensionless (sigmas), and so is robust_scale: rho = u*u, u = s2 / (s2 + e), s2 = scale*scale, on the
 *   28 addends, as "Robust weight"; 0 means no weights.
 *   rslo_surfel_nearest_d: keys_out, d2_out, rows_out as rslo_surfel_nearest; info_out double [N, 8] or NULL: the row
 *   {M00, M01, M02, M11, M12, M22, det, lam} of the matched cell, zeros without a match; for an unusable pair the six
 *   M entries are zeros (det and lam are written as computed).  The table is read-only.
 *   rslo_surfel_normal_eq_d / rslo_surfel_register_d: out29, the two-stage reduction, the step, statuses 0..3, the
 *   converged flag, info rows {status, pairs, cost, |dt|, theta, 0, 0, 0}, the workspace
 *   (rslo_surfel_register_ws_bytes(N)) and the launch counts (2 per iteration, 1 for N == 0) are those of
 *   rslo_surfel_normal_eq / rslo_surfel_register.  Errors are those of the plane calls, plus RSLO_EINVAL for min_flag
 *   outside {1, 2} and for reg_rel / reg_abs that break the rule above (NaN included).
 *
 * Rolling local surfel map (rslo_surfel_prune): the one call that removes surfel cells.  A cell carries no creation
 * scan and the slot layout does not change (156 bytes per slot), so the rule uses only the key, the count
 * N = moments[0], the header's voxel and the arguments.  For a stored cell, cell_a is unpacked from the key (3 x 21
 * bits, x most significant, minus 2^20); then, in this order,
 *   cc_a = (double(cell_a) + 0.5) * voxel      the cell's CENTRE, not the row's mean: a cell with flag 0 (a row of
 *                                              zeros) is judged by where it is
 *   dx = cc_x - c[0], dy, dz likewise;  d2 = dx*dx + dy*dy + dz*dz, summed left to right.
 * The cell is KEPT iff both hold:
 *   1. near:  center3 is NULL, or d2 < radius*radius.  A comparison that is false evicts (a NaN centre coordinate,
 *      radius == 0); radius = +inf keeps every cell.
 *   2. not sparse:  N >= min_count, or (center3 is given and d2 < inner_radius*inner_radius): the sensor's own
 *      neighbourhood is still being filled and is exempt; cells the sensor has left behind that never collected
 *      min_count points -- stray returns, the trails of moving objects -- go.  With center3 == NULL there is no
 *      exemption, and radius and inner_radius are ignored.  min_count = 1 makes nothing sparse.
 * Every other cell is EVICTED: its key, moments and row are gone, rslo_surfel_nearest / _normal_eq / _register /
 * _export do not see it, and a later insert into it starts its moments from zero.  Kept cells keep key, moments and
 * row to the bit (rows are copied, not derived again); all dirty words are 0 afterwards, as between any two calls.
 * n_cells becomes kept - lost, n_planar the number of surviving rows with flag 2.0; n_scans, n_points and the dropped_*
 * counters are cumulative and do not change.  Header words [RSLO_SURFEL_HDR_PRUNE + 0..2] = n_prunes (calls),
 * n_evicted (cumulative), n_lost (cumulative, below); rslo_surfel_reset zeroes them.
 * The table is REBUILT in place, as by rslo_map_prune: the kept records (152 bytes: key, moments, row) are staged in
 * the caller-owned workspace of rslo_surfel_prune_ws_bytes(capacity) bytes (control block | keys | moments | rows),
 * the sections are returned to the state rslo_surfel_reset leaves, and the records are inserted again under the same
 * bounded probe.  A record that finds no empty slot among RSLO_MAP_MAX_PROBE is dropped whole and counted in n_lost:
 * impossible while the survivors' longest run of occupied slots, wrap-around included, is below RSLO_MAP_MAX_PROBE;
 * beyond that the surviving set is unspecified.  A call that evicts nothing leaves every byte of the allocation as it
 * is, except n_prunes.
 *   rslo_surfel_prune_ws_bytes  host only; 0 for a capacity rslo_surfel_bytes refuses.
 *   rslo_surfel_prune  center3: 3 DEVICE doubles (a trajectory row will do) or NULL.  A null map, map_bytes below
 *                    rslo_surfel_bytes(1024), with a centre a radius that is negative or NaN or an inner_radius that
 *                    is negative, NaN or greater than radius, min_count < 1, a null or misaligned (16 bytes)
 *                    workspace: RSLO_EINVAL; ws_bytes below rslo_surfel_prune_ws_bytes of the largest capacity
 *                    map_bytes can hold: RSLO_EWS.  Five launches whatever the data (begin, scan, clear, re-insert,
 *                    done); the scan pass reads keys and counts only and takes the staging cursor once per wave; no
 *                    floating-point atomic.
 *
 * All of them: everything on `stream`, no host read, nothing allocated, a launch count that does not depend on the data:
 * capturable.  On an allocation that was never reset the kernels do nothing (nearest writes "none").  Errors are found
 * before the first launch and write nothing: RSLO_EINVAL for a null pointer, a capacity, size or parameter out of range
 * (NaN included), max_dist outside (0, voxel_size], a bad robust_scale, iters outside 1 .. 32; RSLO_EWS for a workspace
 * below rslo_surfel_insert_ws_bytes(N) / rslo_surfel_register_ws_bytes(N).  The four *_bytes functions are host only
 * and return 0 for arguments out of range.
 * ------------------------------------------------------------------------------------ */
#define RSLO_SURFEL_HDR_PRUNE 15
RSLO_API size_t rslo_surfel_bytes(int64_t capacity);
RSLO_API int rslo_surfel_reset(void *map, size_t map_bytes, int64_t capacity, double voxel_size, double min_range,
                               double max_range, int min_points, double planar_ratio, double line_ratio, void *stream);
RSLO_API size_t rslo_surfel_insert_ws_bytes(int N);
RSLO_API int rslo_surfel_insert(void *map, size_t map_bytes, const float *points, int stride_floats, int N,
                                const double *pose7, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_surfel_insert_frames(void *map, size_t map_bytes, const void *store, size_t store_bytes,
                                       int64_t capacity, int K, const double *poses /*[n_poses,7]*/, int n_poses,
                                       void *stream);
RSLO_API int rslo_surfel_export(const void *map, size_t map_bytes, int min_flag, const double *center3 /*or NULL*/,
                                double radius, uint64_t *keys, int64_t *moments /*[max_rows,10]*/,
                                double *rows /*[max_rows,8]*/, int64_t max_rows, int64_t *counts /*[2]*/, void *stream);
RSLO_API int rslo_surfel_nearest(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                 int stride_floats, int N, const double *pose7, double max_dist, int64_t *keys_out,
                                 double *d2_out, double *rows_out /*[N,8] or NULL*/, void *stream);
RSLO_API size_t rslo_surfel_prune_ws_bytes(int64_t capacity);
RSLO_API int rslo_surfel_prune(void *map, size_t map_bytes, const double *center3 /*device, or NULL*/, double radius,
                               double inner_radius, int min_count, void *ws, size_t ws_bytes, void *stream);
RSLO_API size_t rslo_surfel_register_ws_bytes(int N);
RSLO_API int rslo_surfel_normal_eq(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                   int stride_floats, int N, const double *pose7, double max_dist, double robust_scale,
                                   double *out29, void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_surfel_register(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                  int stride_floats, int N, double *pose7, int iters, double max_dist, double damping,
                                  int min_pairs, double tol_t, double tol_r, double robust_scale, double *info /*[iters,8]*/,
                                  void *ws, size_t ws_bytes, void *stream);
RSLO_API int rslo_surfel_nearest_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                   int stride_floats, int N, const double *pose7, double max_dist, int min_flag,
                                   double reg_rel, double reg_abs, int64_t *keys_out, double *d2_out,
                                   double *rows_out /*[N,8] or NULL*/, double *info_out /*[N,8] or NULL*/, void *stream);
RSLO_API int rslo_surfel_normal_eq_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                     int stride_floats, int N, const double *pose7, double max_dist, int min_flag,
                                     double reg_rel, double reg_abs, double robust_scale, double *out29, void *ws,
                                     size_t ws_bytes, void *stream);
RSLO_API int rslo_surfel_register_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                    int stride_floats, int N, double *pose7, int iters, double max_dist, double damping,
                                    int min_pairs, double tol_t, double tol_r, double robust_scale, int min_flag,
                                    double reg_rel, double reg_abs, double *info /*[iters,8]*/, void *ws, size_t ws_bytes,
                                    void *stream);

/* ------------------------------------------------------------------------------------
 * Scan de-skewing (csrc/deskew.hip; float64 restatement: rslo_amd/deskew.py)
 *
 * A spinning LiDAR does not take a rigid snapshot: while the sweep lasts the sensor moves by M = (t, q).  Under the
 * constant-velocity model of LOAM / LIO-SAM the sensor pose at sweep fraction s in [0, 1] is (s t, R^s), and
 * rslo_deskew moves every point from the sensor frame at its own time to the sensor frame at `stamp`: with stamp = 1 a
 * point seen at s = 0 is moved by M^-1, with stamp = 0 a point seen at s = 1 by M.
 *
 * points fp32 [N, stride_floats], of which n_cols columns are a row: x, y, z, then anything; normal_col (-1: none) is
 * the first of three columns that hold a direction and are rotated with the point.  out fp32 [N, out_stride_floats]
 * receives the n_cols columns; its padding floats are not written.  out == points with equal strides is allowed (a
 * thread reads what it needs of its row before it writes it); any other overlap is the caller's error.
 *
 * The motion is rel7 (DEVICE fp32 [7]: t, q wxyz, widened to double), or se3_between(pose_a, pose_b) = A^-1 o B of two
 * DEVICE double [7] poses, or -- all three NULL -- none.  All pointers are read when the kernel runs: a captured call
 * follows a motion that changes between replays.
 *
 * All arithmetic is IEEE double without contraction, in the order written; the result is rounded to float once, at
 * the store.  rotate is se3_rotate of csrc/se3.h (form A).
 *
 * Motion block (once per call): t = M[0..2], q = M[3..6]; n2 = ((q0*q0 + q1*q1) + q2*q2) + q3*q3.  !(n2 > 0 && n2 < inf)
 * or a component of t not finite: status 2.  Otherwise q /= sqrt(n2), negated when q0 < 0; su = sqrt((q1*q1 + q2*q2) +
 * q3*q3); theta = 2 * atan2(su, q0) -- the only libm transcendental; a = u / su, or 0 when su == 0.  theta > max_angle:
 * status 3.  Otherwise t' = rotate(qs, t) with qs = (cosP(h), sinP(h) * a), h = ((-stamp) * theta) * 0.5.
 *   motion_out double [8] (or NULL) = {a.x, a.y, a.z, theta, t'.x, t'.y, t'.z, status}
 *   status 0 applied, 1 no motion given, 2 invalid motion, 3 angle above max_angle; for a status other than 0 the
 *   first seven words are 0 and every row is copied unchanged, all n_cols floats bit for bit.
 *
 * Per point: s = times[i] (fp32 [N], widened), or the sweep fraction of its azimuth (below).  The row is copied
 * unchanged when x, y, z or s is not finite or, in azimuth mode, when x == 0 && y == 0.  Otherwise s is clamped to
 * [0, 1] and
 *   alpha = s - stamp;  h = (alpha * theta) * 0.5;  qp = (cosP(h), sinP(h) * a)
 *   o = rotate(qp, p) + alpha * t'        (the rotation, then the addition)
 *   the three floats at normal_col become rotate(qp, n); every other column is copied bit for bit.
 *
 * sinP(x) = x * (S1 + z * (S3 + ... + z * S15)), cosP(x) = C0 + z * (C2 + ... + z * C16), z = x*x: the Taylor
 * polynomials in Horner form with the doubles nearest +-1/k!, within 2^-53 of sin and cos for |x| <= pi/4 -- hence
 * max_angle <= pi/2, as |alpha| <= 1.  A fixed polynomial makes the per-point result reproducible to the bit on the host.
 *
 * Sweep fraction from the azimuth: ax = |x|, ay = |y|, r = min(ax, ay) / max(ax, ay); phi = atanP(r); ay > ax:
 * phi = HALF_PI - phi; x < 0: phi = PI - phi; y < 0: phi = -phi; f = phi / TWO_PI - az_start_turn (a division: the
 * axis directions give exact quarters); az_clockwise: f = -f; s = f - floor(f).  atanP(r) = r * (A0 + z * (A1 + ... +
 * z * A8)), z = r*r, with the coefficients of Abramowitz & Stegun 4.4.49 (1, -0.3333314528, 0.1999355085, -0.1420889944,
 * 0.1065626393, -0.0752896400, 0.0429096138, -0.0161657367, 0.0028662257): within 2e-8 rad, 3e-9 of a turn.
 * az_start_turn = -0.5, counter-clockwise, is a sweep that starts and ends at the -x axis.
 *
 * One launch whatever the data (256 threads per workgroup, one thread per row; N == 0: one workgroup that only writes
 * motion_out); every workgroup derives the motion block again (one lane, LDS, a barrier) and workgroup 0 stores it.
 * Everything on `stream`, no host read, no allocation, no atomic: capturable.  Errors are found before the launch and
 * write nothing, RSLO_EINVAL: a null points or out with N > 0, N < 0, n_cols outside 3 .. stride_floats or
 * 3 .. out_stride_floats, a normal_col other than -1 outside 3 .. n_cols - 3, stamp outside [0, 1] or NaN, max_angle
 * outside (0, pi/2], a non-finite az_start_turn, rel7 together with a pose, only one of pose_a and pose_b.
 * ------------------------------------------------------------------------------------ */
RSLO_API int rslo_deskew(const float *points, int stride_floats, int N, int n_cols, int normal_col /* -1: none */,
                         const float *times /* [N] sweep fractions, or NULL: from the azimuth */,
                         const float *rel7 /* device fp32 (t, q wxyz), or NULL */,
                         const double *pose_a, const double *pose_b /* device [7] each, both or neither: motion = A^-1 o B */,
                         double stamp, double az_start_turn, int az_clockwise, double max_angle,
                         float *out, int out_stride_floats, double *motion_out /* device [8], or NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RSLO_HIP_H_ */
