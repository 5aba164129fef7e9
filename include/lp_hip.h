/* lp_hip.h - C ABI of liblp_hip.so: the MI355X (gfx950) kernels behind the Lightning Pose heatmap-tracker
 * training step.
 *
 * The reference (paninski-lab/lightning-pose v2.4.0) is pure Python; the functions below replace the third-party
 * native ops its hot path invokes.  Each entry point cites the reference interface
 * it stands in for (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned, contiguous memory (torch tensor .data_ptr());
 *     the library never allocates, frees or retains pointers; structs are passed by host pointer and only read
 *     during the call
 *   - `stream` is the hipStream_t the kernels are enqueued on (torch.cuda.current_stream().cuda_stream);
 *     calls only enqueue - no device synchronisation, no host read-back
 *   - return value: 0 = LP_OK, < 0 = argument / shape error (nothing was launched), > 0 = hipError_t
 *   - re-entrant and thread-safe: no entry point keeps state between calls or reads the environment.  The only process-wide data is
 *     the table of A/B switches (LP_CONV_PIPE, LP_CONV_HALO, LP_PIPE_WRES, LP_CONV_RES2D, LP_INFER_PIPE, LP_GEMM_PIPE, LP_WGRAD_PIPE,
 *     LP_STEM_2D, LP_STEM_WGRAD_NB, LP_POOL_V2, LP_CONV_MAX_WGS, LP_BN_BWD_WGS_PER_CU), read from the environment ONCE when the library is loaded and immutable afterwards -
 *     except through lp_config_reload_env(), a test / A-B hook that must not run concurrently with other calls
 *   - limits: lp_bn_bwd_apply WITHOUT its terms_ws workspace covers C <= 2048 channels (the per-launch correction table then lives in
 *     LDS; LP_ERR_UNSUPPORTED beyond); with the workspace any C that is a multiple of 8
 *   - heat-maps are fp32 NCHW (B, K, h, w); keypoints are fp32 (B, K, 2) = the reference's (B, 2K) row layout;
 *     backbone activations are bf16 NHWC; weights fp32 masters + bf16 GEMM copies
 */
#ifndef LP_HIP_H
#define LP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lp_stream_t; /* hipStream_t */

/* Re-read the LP_* switches from the environment into the library's switch table (done once, implicitly, at load).  For tests and A/B
 * scripts that flip a switch inside one process; not to be called while another thread is inside an lp_* call. */
int lp_config_reload_env(void);

enum {
    LP_OK = 0,
    LP_ERR_ARGUMENT = -1,    /* null pointer / non-positive dimension  -> ValueError on the Python side */
    LP_ERR_UNSUPPORTED = -2, /* shape outside the instantiated kernels -> NotImplementedError          */
};

enum { LP_TF_NONE = 0, LP_TF_SINGLE = 1, LP_TF_PER_FRAME = 2, LP_TF_PER_VIEW = 3 };

/* ABI version of THIS header: bumped whenever the signature of an existing entry point changes (an argument inserted, a struct field added),
 * not only when symbols come or go.  lp_version() returns the value the library was built with; a caller compares the two before its first
 * call (lightning_pose_amd/_lib.py raises LpHipUnavailable on a mismatch) - a library built against an older header would otherwise take,
 * e.g., the stream argument for an inserted flag without any error.  History: 131 = round 5 (decode `prune`, bn_bwd `terms_ws`), 140 = round 6,
 * 144 = the multi-view token assembly (lp_vit_mv_tokens_*), 145 = the camera geometry of the calibrated 3-D losses (lp_cam_*),
 * 146 = patch masking (lp_patch_mask_f32), 147 = LayerScale inside the LayerNorm walks (lp_layernorm_ls_*, the DINOv2 backbones),
 * 148 = the multi-view labeled batch with its 3-D augmentation (lp_mv3d_*), 149 = lp_conv_last_resident,
 * 150 = the DINOv3 backbones: lp_rope_*, lp_vit_reg_tokens_*, the prefix-dropping lp_layernorm_ls_*_px (and their fp32 forms),
 * 151 = crop-zoom prediction: lp_bbox_from_keypoints, lp_bbox_smooth, lp_frames_crop_resize,
 * 152 = prediction metrics: lp_kp_metrics,
 * 153 = the SAM backbone: lp_window_partition / _unpartition, lp_vit_pos_tokens_*, lp_resid_out_* (and their fp32 forms). */
#define LP_HIP_ABI_VERSION 153
int lp_version(void);
const char* lp_strerror(int code);

/* ------------------------------------------------------------------------------------------------------
 * Decode: heat-map -> sub-pixel keypoints + confidence   (models/heads/heatmap.py:103-144 run_subpixelmaxima,
 * :86-100 upsample, data/heatmaps.py:90-142 evaluate_heatmaps_at_location, data/utils.py:191-234
 * undo_affine_transform_batch, data/bboxes.py:222-288 model_to_frame_batch)
 * ------------------------------------------------------------------------------------------------------ */

/* Banded tap tables of the composite `downsample_factor` x (bicubic x2, 5x5 binomial) operator along each axis,
 * built on the host in fp64 (lightning_pose_amd.ops.decode_tables).  ty = lp_decode_window(ds, h). */
typedef struct lp_decode_tables {
    const int* row_base;     /* [h]           first heat-map row of output-row group j's window                */
    const float* row_taps;   /* [h][R][ty]    taps of output row j*R+rr relative to row_base[j], R = 2^ds        */
    const int* col_start;    /* [w*R]         first heat-map column feeding output column c                    */
    const float* col_taps;   /* [w*R][12]     zero padded                                                      */
    const int* colT_start;   /* [w]           first output column fed by heat-map column q   (backward only)   */
    const float* colT_taps;  /* [w][tc]                                                                        */
    int ty, tx, tc;
} lp_decode_tables;

/* keypoint epilogue: undo the augmentation affine, then model px -> frame px */
typedef struct lp_frame_map {
    const float* transforms; /* LP_TF_SINGLE (2,3) | LP_TF_PER_FRAME (B,2,3) | LP_TF_PER_VIEW (V,2,3) | NULL     */
    int tf_mode;
    const float* bbox;       /* (B, 4*V) rows [x, y, h, w] per view, or NULL for identity                       */
    int bbox_stride;         /* 4*V */
    int kp_per_view;         /* K / V */
    float model_h, model_w;  /* network input size */
} lp_frame_map;

int lp_decode_window(int downsample_factor, int n);

/* `prune` (lp_decode_fwd / lp_decode_bwd): which instantiation of the decode kernels runs - 1 = the exactly-pruned ones (terms below e^-50
 * of the largest are skipped: results equal to the last bit or two, 1.4x / 1.8x faster on the peaked maps of a trained head, slower on flat
 * maps), 0 = the plain ones.  An argument of the call since round 5 (no process state; the product chooses it per model from the decode's
 * own sumexp output, ops.py).  Replaces nothing in the reference (models/heads/heatmap.py:103-144 has one code path). */

/* heat (B,K,h,w) -> kp_aug (B,K,2) model px, kp_frame (B,K,2) frame px, conf (B,K), stats (B,K,4) = {max, sumexp, E[x] - x0, E[y] - y0}: opaque
 * to the caller except [1] (ops.py reads it as "how many pixels carry weight"); (x0, y0) = the up-sampled position of the tile's own maximum, which
 * lp_decode_bwd re-derives from the same tile - the two moments are accumulated about that point (round 6: fp32 resolves offsets of a few pixels
 * 100x finer than coordinates up to 384) */
int lp_decode_fwd(const float* heat, int B, int K, int h, int w, int downsample_factor, float temperature,
                  const lp_decode_tables* tables, const lp_frame_map* frame_map, float* kp_aug, float* kp_frame, float* conf,
                  float* stats, int prune, lp_stream_t stream);

/* g_heat (B,K,h,w) (+)= d loss / d heat given d loss / d kp_aug and/or d loss / d kp_frame (either may be NULL) */
int lp_decode_bwd(const float* heat, int B, int K, int h, int w, int downsample_factor, float temperature,
                  const lp_decode_tables* tables, const lp_frame_map* frame_map, const float* stats, const float* g_kp_aug,
                  const float* g_kp_frame, float* g_heat, int accumulate, int prune, lp_stream_t stream);

/* data/utils.py:191-234 undo_affine_transform_batch + data/bboxes.py:222-288 model_to_frame_batch on their own
 * (target keypoints; backward = 1 applies the transposed Jacobian to a gradient). */
int lp_frame_map_apply(const float* kp_in, int B, int K, const lp_frame_map* frame_map, int backward, float* kp_out,
                       lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Heat-map targets and heat-map losses
 * ------------------------------------------------------------------------------------------------------ */

/* data/heatmaps.py:11-87 generate_heatmaps.  keypoints (B,K,2) image px; visibility int32 (B,K) or NULL. */
int lp_heatmap_gen(const float* keypoints, const int* visibility, int B, int K, int img_h, int img_w, int h, int w, float sigma,
                   float* out, lp_stream_t stream);
/* ... and its gradient with respect to the keypoints (keep_gradients=True, data/heatmaps.py:37-40): grad_keypoints (B,K,2); zero / uniform maps
 * (NaN, out of bounds, visibility < 2) contribute zeros.  Heat-map axes up to 512. */
int lp_heatmap_gen_bwd(const float* keypoints, const int* visibility, int B, int K, int img_h, int img_w, int h, int w, float sigma,
                       const float* grad_out, float* grad_keypoints, lp_stream_t stream);

/* losses/losses.py:706-869 TemporalHeatmapLoss ("temporal_heatmap_mse" = LP_HM_MSE, "temporal_heatmap_kl" = LP_HM_KL): distance
 * between the heat-maps of consecutive frames per keypoint, zeroed where either frame's confidence < prob_threshold, relu(. - epsilon[k]),
 * mean over all (S-1)*K entries.  pred (S,K,h,w), conf (S,K), epsilon (K) device floats; workspace persists to bwd; loss is a device
 * scalar (NaN for S = 1, the mean of an empty tensor).  bwd: gpred (S,K,h,w) = or += gout * d loss / d pred. */
size_t lp_temporal_heatmap_workspace_bytes(int S, int K);
int lp_temporal_heatmap_fwd(int kind, const float* pred, const float* conf, int S, int K, int h, int w, const float* epsilon,
                            float prob_threshold, float* loss, void* workspace, lp_stream_t stream);
int lp_temporal_heatmap_bwd(int kind, const float* pred, int S, int K, int h, int w, const void* workspace, const float* gout,
                            float* gpred, int accumulate, lp_stream_t stream);

/* data/heatmaps.py:90-142 evaluate_heatmaps_at_location: out (B,K) = sum of the (2*radius+1)^2 window of heat (B,K,h,w) around
 * int64(locs (B,K,2) = x, y), zero padded; radius = floor(sigma * num_stds) (2 for the defaults).  The training step gets the
 * same number from lp_decode_fwd's epilogue; this is the standalone form the reference exports. */
int lp_heatmap_confidence(const float* heat, const float* locs, int B, int K, int h, int w, int radius, float* out, lp_stream_t stream);

/* losses/losses.py:229-290,314-335 HeatmapMSELoss (remove_nans -> mse*h*w -> mean).  workspace persists to bwd. */
size_t lp_heatmap_mse_workspace_bytes(int B, int K);
int lp_heatmap_mse_fwd(const float* targ, const float* pred, int B, int K, int h, int w, float* loss, void* workspace,
                       lp_stream_t stream);
int lp_heatmap_mse_bwd(const float* targ, const float* pred, int B, int K, int h, int w, const void* workspace, const float* gout,
                       float* gpred, int accumulate, lp_stream_t stream);
/* The same masked mean for the three supervised heat-map losses: kind = LP_HM_MSE (above), LP_HM_KL (HeatmapKLLoss,
 * losses/losses.py:338-379) or LP_HM_JS (HeatmapJSLoss, :382-423) - kornia's kl_div_loss_2d / js_div_loss_2d of the maps
 * + 1e-10, summed over each map, averaged over the labelled maps.  Workspace as lp_heatmap_mse_workspace_bytes. */
enum { LP_HM_MSE = 0, LP_HM_KL = 1, LP_HM_JS = 2 };
int lp_heatmap_loss_fwd(int kind, const float* targ, const float* pred, int B, int K, int h, int w, float* loss, void* workspace,
                        lp_stream_t stream);
int lp_heatmap_loss_bwd(int kind, const float* targ, const float* pred, int B, int K, int h, int w, const void* workspace,
                        const float* gout, float* gpred, int accumulate, lp_stream_t stream);

/* "unimodal_mse" (not in the reference snapshot; defined by oracle/restated.py unimodal_mse_loss,
 * structurally losses/losses.py:1129-1260).  Same workspace size as lp_heatmap_mse. */
int lp_unimodal_mse_fwd(const float* kp_aug, const float* pred, const float* conf, int S, int K, int img_h, int img_w, int h, int w,
                        float sigma, float prob_threshold, float* loss, void* workspace, lp_stream_t stream);
int lp_unimodal_mse_bwd(const float* kp_aug, const float* pred, int S, int K, int img_h, int img_w, int h, int w, float sigma,
                        const void* workspace, const float* gout, float* gpred, int accumulate, lp_stream_t stream);

/* models/heads/heatmap.py:209-211 spatial_softmax2d(T=1).  Input element (b,k,i) at in[b*sb + i*si + k*sk]. */
int lp_softmax2d_fwd(const float* in, long stride_b, long stride_i, long stride_k, int B, int K, int n, float* out,
                     lp_stream_t stream);
/* gin_bf16: bf16 gradient of the logits in the same strided layout (it feeds the MFMA kernels).  Pixel-major rows (stride_k == 1,
 * stride_i % 8 == 0) are written whole: the pad channels [K, stride_i) of every pixel come out as zeros. */
int lp_softmax2d_bwd(const float* prob, const float* gprob, int B, int K, int n, void* gin_bf16, long stride_b, long stride_i,
                     long stride_k, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Keypoint-space losses (loss scalar + gradient for unit upstream, one launch each)
 * ------------------------------------------------------------------------------------------------------ */

/* losses/losses.py:576-703 TemporalLoss.  kp (S,K,2), conf (S,K) or NULL, eps_per_kp (K). */
int lp_temporal_fwd_bwd(const float* kp, const float* conf, int S, int K, const float* eps_per_kp, float prob_threshold,
                        float* loss, float* grad_unit, lp_stream_t stream);

/* losses/losses.py:528-573 PCALoss + utils/pca.py:97-190,266-309.  index (rows, points) int32 keypoint ids. */
int lp_pca_fwd_bwd(const float* kp, int S, int K, const int* index, int rows, int points, const float* mean,
                   const float* kept_eigenvectors, int ncomp, float epsilon, float* loss, float* grad_unit, lp_stream_t stream);

/* losses/losses.py:880-996 RegressionRMSELoss (always-on diagnostic, models/base.py:528). */
int lp_rmse_fwd(const float* kp_targ, const float* kp_pred, int n_points, float* loss, lp_stream_t stream);
/* LossFactory.__call__ (reference losses/factory.py:229-285) in one launch: weighted[i] = w[i] * x[i][0] (logged as "<stage>_<name>_loss_weighted"),
 * total = sum_i a[i] * weighted[i] in registry order (a = the anneal value for the unsupervised terms, 1 for the heat-map losses).  x: HOST array of
 * n <= 8 DEVICE scalars; w, a: host arrays.  _bwd: gx[i] = w[i] * (g_weighted[i] + a[i] * g_total[0]); either gradient may be NULL. */
int lp_loss_combine(const float* const* x, const float* w, const float* a, int n, float* weighted, float* total, lp_stream_t stream);
int lp_loss_combine_bwd(const float* w, const float* a, int n, const float* g_weighted, const float* g_total, float* gx, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Prediction metrics (csrc/metrics.hip; reference metrics.py:47-184, losses/losses.py:651-672, utils/pca.py:266-309): up to four (T, K)
 * fp32 tables from a device-resident prediction table in ONE launch on the caller's stream; nothing is read back.
 *   pred (T, K, 2); labels (T, K, 2) or NULL.  An output pointer that is NULL is a table that is not wanted (at least one must be given).
 *   pixel_error[t,k]   = ||labels[t,k] - pred[t,k]||                      (needs labels; NaN where a coordinate of either is NaN)
 *   temporal_norm[t,k] = ||pred[t,k] - pred[t-1,k]|| for t >= 1, NaN for t = 0   (no epsilon, no confidence mask, no relu)
 *   pca_singleview[t,k]: frame t is one sample over the `points` keypoints of the index row; keypoint index[p] gets the Euclidean norm of
 *       its 2-D residual (x - mean) - V^T V (x - mean), every other column NaN.  rows must be 1.
 *   pca_multiview[t,k]: sample (t, j) gathers keypoints index[j][0 .. points) (one per view); their residual norms go to those columns,
 *       every other column NaN.
 *   A NaN coordinate in a PCA sample makes every entry of that sample NaN (the reference's matmul); +-Inf is not specified.  A column that
 *   an index table lists more than once takes the value of its LAST entry (numpy's fancy assignment).
 * lp_pca_spec: index (rows, points) int32 as KeypointPCA.index_table builds it for lp_pca_fwd_bwd, on the DEVICE, and index_host, the same
 * table in HOST memory: it is checked before the launch.  mean (2 points), kept_eigenvectors (ncomp, 2 points): device fp32.
 * Every element of every requested table is written exactly once (the NaN fills too): no memset beforehand, no atomics, no workspace, and
 * the same bits from run to run and for any launch geometry.
 * LP_ERR_ARGUMENT (nothing launched): a null pred, T or K < 1, no output, pixel_error without labels, a PCA output without its spec,
 *   points > 64, ncomp > 2 points, ncomp < 0, an index_host entry outside [0, K), rows != 1 for the single-view spec, rows points > 2^24.
 * LP_ERR_UNSUPPORTED (nothing launched): 2 T K >= 2^31 elements, or eigenvectors + owner maps ((ncomp 2 points + K) words per requested
 *   PCA table) beyond the 160 KB of one workgroup's LDS.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct lp_pca_spec {
    const int* index;               /* device (rows, points) */
    const int* index_host;          /* host copy of the same table */
    int rows, points;
    const float* mean;              /* device (2 points) */
    const float* kept_eigenvectors; /* device (ncomp, 2 points) */
    int ncomp;
} lp_pca_spec;
int lp_kp_metrics(const float* pred, const float* labels, int T, int K, const lp_pca_spec* singleview, const lp_pca_spec* multiview,
                  float* pixel_error, float* temporal_norm, float* pca_singleview, float* pca_multiview, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Backbone / head contractions on the matrix cores (bf16 NHWC activations, fp32 accumulate).
 * Replace cuDNN behind `self.backbone(images)` (models/base.py:398; models/backbones/factory.py:322-325) and
 * nn.ConvTranspose2d in the head (models/heads/heatmap.py:60-69).  A ConvTranspose2d(k3,s2,p1,op1) forward is
 * lp_conv_dgrad of the mirrored convolution, its data-gradient is lp_conv_fwd, its weight-gradient lp_conv_wgrad.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct lp_conv_geom {
    int B, Hi, Wi, Ci; /* input  tensor, NHWC */
    int Ho, Wo, Co;    /* output tensor, NHWC */
    int R, S, stride, pad;
} lp_conv_geom;

/* Which kernel family the most recent convolution entry point called from this thread launched: conv_igemm_kernel (register-staged,
 * 128-row tiles), conv_pipe_kernel (direct-to-LDS ring, 256-row tiles; LP_CONV_PIPE=0 disables it), or the two weight-gradient kernels.
 * Diagnostic only (bench labels, tests); replaces nothing in the reference. */
#define LP_CONV_KERNEL_IGEMM 0
#define LP_CONV_KERNEL_PIPE 1
#define LP_CONV_KERNEL_WGRAD 2
#define LP_CONV_KERNEL_WGRAD_PIPE 3
#define LP_CONV_KERNEL_PIPE_HALO 4 /* conv_pipe_kernel<..., HALO>: 3x3 / stride 1, the input neighbourhood staged once (LP_CONV_HALO=0 disables) */
/* (6, 7: round 5's producer / consumer kernel conv_spec_kernel - measured not faster, retired in round 6: profiles/retired/r05_conv_spec.h.txt) */
#define LP_CONV_KERNEL_STEM_WGRAD_NB 8 /* stem_wgrad_nb_kernel: the stem's weight gradient from a staged input neighbourhood (LP_STEM_WGRAD_NB=0 disables) */
#define LP_CONV_KERNEL_WGRAD_NB 9 /* conv_wgrad_nb_kernel: 3x3 / stride 1 weight gradient, input staged once for all nine taps (LP_WGRAD_NB=0 disables) */
#define LP_CONV_KERNEL_RES2D 5     /* conv_res2d_kernel: 3x3 / stride 1, 64 -> 64 channels, 16 x 16 tiles, filter resident in LDS (LP_CONV_RES2D=0 disables) */
int lp_conv_last_kernel(void);
/* 1 if that launch was conv_pipe_kernel's weight-resident form (1x1 / stride 1 with K * column block * 2 <= 64 KB: the weight panel stays
 * in LDS for the workgroup's whole walk; LP_PIPE_WRES=0 disables it, =2 takes it wherever the shape allows), else 0.  The kernel id above
 * stays LP_CONV_KERNEL_PIPE for it.  Diagnostic only. */
int lp_conv_last_resident(void);

/* w: bf16 [Co][R][S][Ci] (Ci % 64 == 0).  Output row-major [B*Ho*Wo][ldo], columns < n_store written. */
int lp_conv_fwd(const void* x, const void* w, const lp_conv_geom* geom, const float* bias, void* out_bf16, float* out_f32, int ldo,
                int n_store, lp_stream_t stream);
/* wd: bf16 [Ci][R][S][Co] (Co % 64 == 0); optional bf16 addend (same layout as dx) is summed in; optional relu_mask (the
 * bf16 activation dx is the gradient of) zeroes dx where the activation is <= 0, i.e. the ReLU backward is fused here.
 * addend may alias dx (in-place accumulation).  A stride-2 gradient runs as 4 parity-class launches; with skip_empty_classes the
 * classes no filter tap reaches (3 of 4 for a 1x1) are not touched - use it when dx already holds addend there. */
int lp_conv_dgrad(const void* dy, const void* wd, const lp_conv_geom* geom, const float* bias, const void* addend,
                  const void* relu_mask, void* dx_bf16, float* dx_f32, int ldo, int n_store, int skip_empty_classes,
                  lp_stream_t stream);
/* The forward kernel as a plain NT GEMM (the token-wise Linear layers and the attention products of the ViT backbone,
 * models/backbones/vit.py:16-49 -> transformers ViTModel):  C[z][m][n] = sum_k A[z][m][k] * B[z][n][k] (+ bias[n]).
 * A: bf16 rows of pitch lda, B: bf16 rows of pitch ldb (K % 64 == 0, pitches % 8 == 0), C: bf16 or fp32 rows of pitch ldc.
 * Columns n < n_store are written (n_store may exceed N up to the tile: the extra columns repeat row N-1 of B); with n_store a
 * multiple of 8 and bf16 output the coalesced store path is taken.  `batch` (optional): nb x nh independent products whose
 * operands start at a_b*zb + a_h*zh (elements; likewise b_*, c_*), e.g. per (image, head) slices of a fused QKV tensor. */
typedef struct lp_gemm_batch {
    int nb, nh;
    long long a_b, a_h, b_b, b_h, c_b, c_h;
} lp_gemm_batch;
int lp_gemm_nt(const void* a, int lda, const void* b, int ldb, void* c_bf16, float* c_f32, int ldc, int M, int N, int K, int n_store,
               const float* bias, const lp_gemm_batch* batch, lp_stream_t stream);
/* out[z][j][n] (bf16, pitch ldo) = sum_m x[z][m][j] * y[z][m][n]: both operands are contracted over their ROW index (the
 * weight-gradient kernel used directly; attention's dV = P^T dO and dK = dS^T Q).  batch: a_* = x, b_* = y, c_* = out strides. */
int lp_gemm_tn(const void* x, int ldx, const void* y, int ldy, void* out_bf16, int ldo, int M, int J, int N, const lp_gemm_batch* batch,
               lp_stream_t stream);
/* Fused soft-max attention forward, head dimension 64 (HF ViTSelfAttention eager attention, reference models/backbones/vit.py:38-43):
 * per (image b, head h):  P = softmax(scale * Q K^T) -> p_bf16[(b*nh + h)*T + q][ldp] (pad columns [T, ldp) zeroed; the backward pass
 * reads it),  O = P V -> out_bf16[(b*T + q)*ldo + h*64 ..].  Token rows qkv_bf16[(b*T + t)*ld_qkv + ..] hold Q at column h*64, K at
 * k_off + h*64 and V at v_off + h*64.  The scores stay on chip (two passes over the keys: running max / exp-sum, then P and O).
 * p_bf16 == NULL (inference): P is used for O and dropped - nothing of size T x T is written. */
int lp_attn_fwd(const void* qkv_bf16, int ld_qkv, int k_off, int v_off, int B, int nh, int T, float scale, void* p_bf16, int ldp,
                void* out_bf16, int ldo, lp_stream_t stream);
/* Attention backward, key / value side, in one pass over the stored probabilities (the autograd of HF ViTSelfAttention's eager
 * attention, reference models/backbones/vit.py:38-43 -> transformers ViTModel; replaces lp_attn_dscores + 2 x lp_gemm_tn):
 *   dS[z][q][k] = scale * P[z][q][k] * (sum_d dO[q][d] V[k][d] - D[q])   -> ds_bf16 (layout / pitch of P, pad columns zeroed; dQ = dS K reads it)
 *   dV[k][d] = sum_q P[q][k] dO[q][d]  -> dqkv_bf16[(b*T + k)*ld_dqkv + dv_off + h*64 + d]
 *   dK[k][d] = sum_q dS[q][k] Q[q][d]  -> dqkv_bf16[(b*T + k)*ld_dqkv + dk_off + h*64 + d]
 * Q / V come from the token rows of lp_attn_fwd, dO from d_out_bf16[(b*T + q)*ld_do + h*64 ..], D = lp_attn_rowdot's [B*T][nh]. */
int lp_attn_bwd_kv(const void* qkv_bf16, int ld_qkv, int v_off, const void* d_out_bf16, int ld_do, const void* p_bf16, int ldp, const float* d_rows,
                   int B, int nh, int T, float scale, void* ds_bf16, void* dqkv_bf16, int ld_dqkv, int dk_off, int dv_off, lp_stream_t stream);
/* Attention backward without materialising dP (replaces lp_gemm_nt + lp_softmax_rows_bwd of the composition; the reference's
 * arithmetic is HF ViTSelfAttention's eager soft-max attention, models/backbones/vit.py:38-43):
 *   lp_attn_rowdot   D[row][h] = sum_d a[row][h*64+d] * b[row][h*64+d]   (a = dO, b = O, head dimension 64)
 *   lp_attn_dscores  dS[z][m][n] = scale * P[z][m][n] * (sum_k dO[z][m][k] V[z][n][k] - D[z][m]), pad columns [N, ldc) zeroed;
 *                    P has the layout of dS; D[z][m] sits at d_rows[zb*d_b + zh*d_h + m*d_row_stride]; batch as in lp_gemm_nt. */
int lp_attn_rowdot(const void* a_bf16, const void* b_bf16, int rows, int nh, int ld, float* out, lp_stream_t stream);
int lp_attn_dscores(const void* d_out, int ld_do, const void* v, int ldv, const void* p_bf16, const float* d_rows, int d_row_stride,
                    long long d_b, long long d_h, float scale, void* ds_bf16, int ldc, int M, int N, int K, const lp_gemm_batch* batch,
                    lp_stream_t stream);
/* A BatchNorm sum in FIXED POINT (round 4): value = hi * 2^-12 + lo * 2^-60.  The reductions over rows that are spread across workgroups -
 * the sums the convolution store passes take, lp_bn_pool_bwd_reduce - split each workgroup's fp32 partial sum t into hi = rint(t 2^12),
 * lo = rint((t - hi 2^-12) 2^60) and add both with 64-bit INTEGER atomics (lp_bn_stats / lp_bn_bwd_reduce: per-workgroup fp32 rows added in
 * a fixed order, then one such addition per channel).  Integer addition commutes, so
 * the totals do not depend on the order in which workgroups arrive: a training step repeats bit for bit (the reference is deterministic on
 * a fixed seed, models/heatmap_tracker.py:69-70; rounds 2 - 3 used fp32 atomics and did not).  |sum| < 2^50; a partial of magnitude
 * >= 1e-10 is represented exactly, smaller ones to 4e-19.  Buffers are accumulated into: zero them first.  SyncBatchNorm all-reduces the
 * integers (SUM is exact).  lp_bn_finalize / lp_bn_bwd_apply / lp_bn_pool_bwd_apply read them. */
typedef struct lp_fxsum {
    long long hi, lo;
} lp_fxsum;
/* The data gradient of a Linear layer that follows a GELU, leaving as the gradient of the GELU's INPUT (a ViT block's fc2 -> fc1's
 * output; HF ViTIntermediate / ViTOutput, reference models/backbones/vit.py:29-49 through transformers' ViTLayer):
 *   c[m][n] = bf16( bf16(sum_k a[m][k] * b[n][k]) * GELU'(u[m][n]) ),   a (M, K), b (N, K), u and c (M, N), all dense bf16;
 * the inner rounding is the one lp_gemm_nt's output would have had, so the result equals lp_gemm_nt followed by lp_gelu_bwd bit for
 * bit, without the activation gradient's write and read.  colsum (optional, (2, N) lp_fxsum, zeroed by the caller): row 0 receives the
 * column sums of c - the bias gradient of the layer that produced u (lp_fxsum_accumulate turns them into fp32); row 1 is scratch.
 * LP_ERR_UNSUPPORTED unless K % 64 == 0 and N % 128 == 0 (the pipelined kernel's shapes): the caller then runs the two-pass form. */
int lp_gemm_nt_gelu_bwd(const void* a, const void* b, const void* u_bf16, void* c_bf16, int M, int N, int K, lp_fxsum* colsum,
                        lp_stream_t stream);
/* ... and the forward side of the same pair: c = bf16(a b^T + bias) as lp_gemm_nt writes it, and act = bf16(GELU(c)) beside it (what
 * lp_gelu_fwd would compute from c, bit for bit): fc1 of a ViT block leaves with its activation.  Same shape limits. */
int lp_gemm_nt_gelu_fwd(const void* a, const void* b, const float* bias, void* c_bf16, void* act_bf16, int M, int N, int K,
                        lp_stream_t stream);
/* BatchNorm reductions fused into the store pass of the convolution next to it, so the normalised tensor is not re-read
 * for them (torch.nn.BatchNorm2d training forward / backward).  Every persistent workgroup adds the
 * column sums of the tiles it walked into `sums` (fixed point, integer atomics: see lp_fxsum).
 *   lp_conv_fwd_bn / lp_stem_fwd_bn:  sums (2,Co) += [sum z, sum z^2] of the bf16 output z  (== lp_bn_stats on it);
 *                                     only sums / seg_images are read.
 *   lp_conv_dgrad_bn:                 dx is the gradient of a = relu(BN(z) [+ residual]); sums (2,Ci) += [sum dx, sum dx*xhat]
 *                                     (== lp_bn_bwd_reduce; the BatchNorm's d beta / d gamma ARE these sums: lp_bn_bwd_apply adds them
 *                                     into the parameter gradients).
 *                                     mask_from_z = 1 recomputes the ReLU mask as bf16(gamma*invstd*(z-mean)+beta) > 0 (layers
 *                                     without a residual branch; relu_mask must then be NULL), otherwise pass relu_mask or
 *                                     bn->relu_bits. */
typedef struct lp_bn_fuse {
    const void* z;        /* bf16 [rows][C] pre-normalisation tensor (dgrad only) */
    const float* mean;    /* (C,) batch mean      (dgrad only) */
    const float* invstd;  /* (C,) 1/sqrt(var+eps) (dgrad only) */
    const float* gamma;   /* (C,) weight, mask_from_z only */
    const float* beta;    /* (C,) bias,   mask_from_z only */
    int mask_from_z;
    const void* relu_bits; /* dgrad only, optional: 1-bit ReLU mask written by lp_bn_apply (then relu_mask must be NULL) */
    lp_fxsum* sums;       /* (2,C) fixed-point sums, accumulated into (zero first) */
    /* Two BatchNorm segments in ONE launch: images [0, seg_images) and [seg_images, B) keep separate batch statistics - the labeled
     * and the unlabeled frames of a semi-supervised step, which the reference normalises in two forward calls (models/base.py:682-695).
     * Then sums is (2 segments, 2, C), mean / invstd are (2, C).  seg_images times the
     * launch's rows per image must be a multiple of 128 (LP_ERR_UNSUPPORTED otherwise: run the segments as two calls).  0 = one segment. */
    int seg_images;
    /* lp_conv_dgrad_bn only (stride 1, relu_bits given): `addend` is the data gradient of the block's stride-2 projection shortcut on ITS grid,
     * [B][ceil(Hi / 2)][ceil(Wi / 2)][Ci] bf16, added at the pixels with even row and column only - the projection shortcut then needs no
     * read-modify-write pass over dx and this launch, the last writer, can take the BatchNorm sums (round 5).  0 = a dense addend. */
    int addend_half;
} lp_bn_fuse;
/* lp_conv_dgrad (bf16 result, no bias) with the ReLU mask read at 1 BIT per element - relu_bits[(row * Ci + c) / 8] bit c % 8, the bytes
 * lp_bn_apply writes beside the activation - instead of from the bf16 activation itself (round 5: the two data gradients into a layer's first
 * block's input read 1/16 of the mask bytes).  Results are identical to lp_conv_dgrad(relu_mask = that activation).
 * Reference: autograd of relu(bn3(z) + identity) feeding conv1 / downsample under models/base.py:398. */
int lp_conv_dgrad_bits(const void* dy, const void* wd, const lp_conv_geom* geom, const void* addend, const void* relu_bits, void* dx_bf16,
                       int skip_empty_classes, lp_stream_t stream);
/* Inference (predict_step, models/heatmap_tracker.py:155-191; eval-mode nn.BatchNorm2d uses its running statistics): the BatchNorm
 * after a convolution is folded into it once per set of weights - lp_bn_fold: w_bf16[co][:] = bf16(w[co][:] * a[co]),
 * bias[co] = beta[co] - running_mean[co] * a[co], a = gamma / sqrt(running_var + eps) - and the layer becomes ONE launch,
 * lp_conv_fwd_act: out = [relu](conv(x, w_bf16) + bias + residual), residual = the block's identity / shortcut (bf16, layout of out)
 * or NULL.  No BatchNorm pass, no pre-normalisation tensor, nothing kept for a backward pass.  Runs on conv_pipe_kernel<.., kEkInfer> where
 * the training forward would (LP_INFER_PIPE=0: conv_igemm_kernel<infer>); there the residual and the ReLU act on bf16(accumulator + bias). */
int lp_bn_fold(const float* w, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
               int Co, int per_co, void* w_bf16, float* bias, lp_stream_t stream);
int lp_conv_fwd_act(const void* x, const void* w, const lp_conv_geom* geom, const float* bias, const void* residual_bf16, int relu,
                    void* out_bf16, lp_stream_t stream);
int lp_conv_fwd_bn(const void* x, const void* w, const lp_conv_geom* geom, void* out_bf16, const lp_bn_fuse* bn, lp_stream_t stream);
int lp_stem_fwd_bn(const void* x4, const void* w, const lp_conv_geom* geom, void* out_bf16, const lp_bn_fuse* bn, lp_stream_t stream);
int lp_conv_dgrad_bn(const void* dy, const void* wd, const lp_conv_geom* geom, const void* addend, const void* relu_mask,
                     void* dx_bf16, const lp_bn_fuse* bn, lp_stream_t stream);
/* dw: fp32 [Co][R][S][Ci], accumulated into (zero it first); split_hint <= 0 picks the pixel split.  The pixel slices leave
 * partial tiles in `workspace` (lp_conv_wgrad_workspace_bytes) and a second kernel sums them in a fixed order: deterministic.
 * lp_conv_wgrad_workspace_bytes(geom, split_hint) suffices for the same geom and split_hint whichever kernel the LP_* switches route
 * the launch to.  A workspace smaller than the routed kernel's plan needs is LP_ERR_ARGUMENT, returned before anything is launched
 * (lp_conv_wgrad, lp_conv_wgrad_bias, lp_stem_wgrad): the library does not fall back to a slower kernel with a smaller plan. */
size_t lp_conv_wgrad_workspace_bytes(const lp_conv_geom* geom, int split_hint);
int lp_conv_wgrad(const void* x, const void* dy, const lp_conv_geom* geom, float* dw, int split_hint, void* workspace,
                  size_t workspace_bytes, lp_stream_t stream);
/* same, plus dbias[co] += sum_m dy[m][co] (bias gradient of a Linear layer of the ViT backbone, reference models/backbones/vit.py:16-49,
 * or of a ConvTranspose2d of the head, models/heads/heatmap.py:20-71) out of the same pass over dy: fp32
 * atomics, one per column and pixel slice, so the summation order (not the set of addends) can vary between runs */
int lp_conv_wgrad_bias(const void* x, const void* dy, const lp_conv_geom* geom, float* dw, float* dbias, int split_hint, void* workspace,
                       size_t workspace_bytes, lp_stream_t stream);
/* ResNet stem 7x7/2: x4 = NHWC4 bf16 (channel 3 zero), weights / gradients in the padded [64][8][8][4] layout. */
int lp_stem_fwd(const void* x4, const void* w, const lp_conv_geom* geom, void* out_bf16, lp_stream_t stream);
int lp_stem_wgrad(const void* x4, const void* dy, const lp_conv_geom* geom, float* dw, int split_hint, void* workspace,
                  size_t workspace_bytes, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * fp32 VALIDATION path (csrc/fp32.hip): the same layers in fp32 end to end on v_mfma_f32_32x32x2_f32, so a whole training step can
 * be held against the reference - which trains in fp32 only (lightning_pose/train.py:411-428 passes no precision) - at the 1e-4
 * tolerance BASELINE.json's north_star states for fp32.  Untuned (scalar operand loads, one wave per 32 x 32 tile): it exists to
 * prove the wiring, the bf16-mixed entry points above are the product and the measured path.
 * Tensors are dense NHWC fp32; weights are read straight from the flat fp32 parameter buffer in its [Co][KH][KW][CiS] storage
 * (KH, KW, CiS >= R, S, Ci: the stem is stored [64][8][8][4]); dgrad needs no transposed copy.  `addend` (may alias the output) is
 * added to the result; lp_f32_conv_wgrad accumulates into dw with fp32 atomics.
 * ------------------------------------------------------------------------------------------------------ */
int lp_f32_conv_fwd(const float* x, const float* w, const lp_conv_geom* geom, int KH, int KW, int CiS, const float* bias,
                    const float* addend, float* out, lp_stream_t stream);
int lp_f32_conv_dgrad(const float* dy, const float* w, const lp_conv_geom* geom, int KH, int KW, int CiS, const float* bias,
                      const float* addend, float* dx, lp_stream_t stream);
int lp_f32_conv_wgrad(const float* x, const float* dy, const lp_conv_geom* geom, int KH, int KW, int CiS, float* dw, lp_stream_t stream);
/* fp32 forms of lp_bn_stats / lp_bn_apply / lp_bn_bwd_reduce / lp_bn_bwd_apply (lp_bn_finalize is shared), of the 3x3/2 max-pool, of the
 * input layout conversion (NCHW -> NHWC4), of PixelShuffle(2) and of the spatial soft-max backward (fp32 gradient out) */
int lp_f32_bn_stats(const float* x, int M, int C, float* sums, lp_stream_t stream);
/* the same sums through per-stripe partials in `workspace`, added in a fixed order (no atomics): the validation executor's forward statistics,
 * so that its outputs repeat bit for bit from run to run */
size_t lp_f32_bn_stats_workspace_bytes(int M, int C);
int lp_f32_bn_stats_ordered(const float* x, int M, int C, float* sums, void* workspace, size_t workspace_bytes, lp_stream_t stream);
int lp_f32_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* residual,
                    int relu, int M, int C, float* y, lp_stream_t stream);
int lp_f32_bn_bwd_reduce(const float* dy, const float* y_out, const float* x, const float* mean, const float* invstd, int M, int C,
                         float* sums, float* dbeta_acc, float* dgamma_acc, lp_stream_t stream);
int lp_f32_bn_bwd_apply(const float* dy, const float* y_out, const float* x, const float* mean, const float* invstd, const float* gamma,
                        const float* sums, float count, int M, int C, float* dx, float* dres, lp_stream_t stream);
int lp_f32_maxpool_fwd(const float* x, int B, int Hi, int Wi, int C, float* y, void* argmax_u8, lp_stream_t stream);
int lp_f32_maxpool_bwd(const void* argmax_u8, const float* dy, int B, int Hi, int Wi, int C, float* dx, lp_stream_t stream);
int lp_f32_images_to_nhwc4(const float* images, int B, int H, int W, float* out, lp_stream_t stream);
int lp_f32_pixel_shuffle(const float* in, int B, int h, int w, int c_out, int ld, int inverse, float* out, lp_stream_t stream);
int lp_f32_softmax2d_bwd(const float* prob, const float* gprob, int B, int K, int n, float* gin, long stride_b, long stride_i, long stride_k,
                         lp_stream_t stream);
/* fp32 forms of the ViT-S/16 glue (csrc/vit_f32.hip) - patch rows, token assembly, LayerNorm (+ residual add in front, [CLS] rows dropped
 * with drop_T), exact GELU - and of the attention over the fused qkv tensor (head dimension 64; p [B][nh][T][T] keeps the probabilities,
 * ds_workspace the same size): config C4 (lightning_pose/models/backbones/vit.py:16-49 over HuggingFace ViTModel) at the reference's own
 * precision.  The Linear layers of that path are lp_f32_conv_fwd / _dgrad / _wgrad with a 1x1 geometry. */
int lp_f32_vit_patchify(const float* images, int B, int H, int W, int patch, float* out, lp_stream_t stream);
int lp_f32_vit_tokens_fwd(const float* patch, const float* cls, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream);
int lp_f32_vit_tokens_bwd(const float* dx, int B, int Np, int D, float* dpatch, float* dpos, lp_stream_t stream);
/* fp32 forms of lp_vit_mv_tokens_fwd / _bwd (below): patch and dpatch in float, the same workspace (lp_vit_mv_tokens_bwd_workspace_bytes) */
int lp_f32_vit_mv_tokens_fwd(const float* patch, const float* pos, const float* view, int B, int V, int Np, int D, float* x, lp_stream_t stream);
int lp_f32_vit_mv_tokens_bwd(const float* dx, int B, int V, int Np, int D, float* dpatch, float* dpos, float* dview, void* workspace,
                             size_t workspace_bytes, lp_stream_t stream);
/* as lp_layernorm_fwd (below) with delta, y in fp32 and any D, except: with delta == NULL x_out is ignored and left unwritten (the
 * normalised tensor is x itself); with a delta x_out is required and may alias x */
int lp_f32_layernorm_fwd(const float* x, const float* delta, float* x_out, const float* gamma, const float* beta, float eps, int M, int D,
                         int drop_T, float* y, float* mean, float* rstd, lp_stream_t stream);
int lp_f32_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, int M, int D, int drop_T,
                         float* dx_acc, float* dgamma_acc, float* dbeta_acc, lp_stream_t stream);
/* the fp32 forms of lp_layernorm_ls_fwd / _bwd (below): delta / branch / dy fp32, dx_out = ls o (updated dx_acc) unrounded */
int lp_f32_layernorm_ls_fwd(const float* x, const float* delta, const float* ls, float* x_out, const float* gamma, const float* beta, float eps,
                            int M, int D, int drop_T, float* y, float* mean, float* rstd, lp_stream_t stream);
int lp_f32_layernorm_ls_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* ls,
                            const float* branch, int M, int D, int drop_T, float* dx_acc, float* dx_out, float* dgamma_acc, float* dbeta_acc,
                            float* colsum_acc, float* dls_acc, lp_stream_t stream);
/* the fp32 forms of lp_layernorm_ls_fwd_px / _bwd_px, lp_rope_fwd / _bwd and lp_vit_reg_tokens_fwd / _bwd (below): float rows, the same table */
int lp_f32_layernorm_ls_fwd_px(const float* x, const float* delta, const float* ls, float* x_out, const float* gamma, const float* beta,
                               float eps, int M, int D, int drop_T, int n_prefix, float* y, float* mean, float* rstd, lp_stream_t stream);
int lp_f32_layernorm_ls_bwd_px(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* ls,
                               const float* branch, int M, int D, int drop_T, int n_prefix, float* dx_acc, float* dx_out, float* dgamma_acc,
                               float* dbeta_acc, float* colsum_acc, float* dls_acc, lp_stream_t stream);
int lp_f32_rope_fwd(float* qkv, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh,
                    int head_dim, lp_stream_t stream);
int lp_f32_rope_bwd(float* dqkv, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh,
                    int head_dim, lp_stream_t stream);
int lp_f32_vit_reg_tokens_fwd(const float* patch, const float* cls, const float* reg, int B, int R, int Np, int D, float* x, lp_stream_t stream);
int lp_f32_vit_reg_tokens_bwd(const float* dx, int B, int R, int Np, int D, float* dpatch, float* dcls, float* dreg, lp_stream_t stream);
/* the fp32 forms of lp_window_partition / _unpartition, lp_vit_pos_tokens_fwd / _bwd and lp_resid_out_fwd / _bwd (below): float rows;
 * the residual add has no y (the features are x_out itself) */
int lp_f32_window_partition(const float* src, int ld_src, int B, int gh, int gw, int ws, int cols, const float* fill, float* dst,
                            lp_stream_t stream);
int lp_f32_window_unpartition(const float* src, int B, int gh, int gw, int ws, int cols, float* dst, int ld_dst, float* pad_colsum_acc,
                              lp_stream_t stream);
int lp_f32_vit_pos_tokens_fwd(const float* patch, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream);
int lp_f32_vit_pos_tokens_bwd(const float* dx, int B, int Np, int D, float* dpatch, float* dpos, lp_stream_t stream);
int lp_f32_resid_out_fwd(const float* x, const float* delta, size_t n, float* x_out, lp_stream_t stream);
int lp_f32_resid_out_bwd(const float* dy, size_t n, float* dx, lp_stream_t stream);
int lp_f32_gelu_fwd(const float* x, size_t n, float* y, lp_stream_t stream);
int lp_f32_gelu_bwd(const float* x, const float* dy, size_t n, float* dx, lp_stream_t stream);
int lp_f32_attn_fwd(const float* qkv, int ld, int k_off, int v_off, int B, int nh, int T, float scale, float* p, float* o, int ldo,
                    lp_stream_t stream);
int lp_f32_attn_bwd(const float* qkv, int ld, int k_off, int v_off, const float* dout, int ldo, const float* p, int B, int nh, int T,
                    float scale, float* ds_workspace, float* dqkv, int ldd, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * HBM-bound glue of the trunk (NHWC bf16): BatchNorm2d training mode, ReLU, residual add, MaxPool2d(3,2,1),
 * PixelShuffle(2), input layout.  torchvision Bottleneck semantics; called from
 * `self.backbone(images)` (models/base.py:398) and HeatmapHead.forward (models/heads/heatmap.py:44,208).
 * ------------------------------------------------------------------------------------------------------ */
/* sums (2,C) fixed point (lp_fxsum), accumulated into (zero first): [sum x, sum x^2] over the M rows.  SyncBatchNorm = all-reduce it
 * (int64 SUM).  `workspace` (lp_bn_reduce_workspace_bytes; also for lp_bn_bwd_reduce): one fp32 row of partial sums per workgroup, added in
 * a fixed order by a second launch - up to 1024 workgroups finish together here, too many for atomics on one address each. */
size_t lp_bn_reduce_workspace_bytes(int M, int C);
int lp_bn_stats(const void* x, int M, int C, lp_fxsum* sums, void* workspace, size_t workspace_bytes, lp_stream_t stream);
/* dst[i] += value of sums[i], i < n (fixed-point totals as fp32) */
int lp_fxsum_accumulate(const lp_fxsum* sums, int n, float* dst, lp_stream_t stream);
int lp_bn_finalize(const lp_fxsum* sums, float count, int C, float eps, float momentum, float* mean, float* invstd,
                   float* running_mean, float* running_var, lp_stream_t stream);
/* the same from plain fp32 [sum, sum of squares] (the fp32 validation executor: lp_f32_bn_stats_ordered) */
int lp_bn_finalize_f32(const float* sums, float count, int C, float eps, float momentum, float* mean, float* invstd,
                       float* running_mean, float* running_var, lp_stream_t stream);
/* two segments at once: sums (2,2,C), mean / invstd (2,C); the running statistics take segment 0's update, then segment 1's - the
 * order of the reference's two forward calls (labeled, then unlabeled: models/base.py:682-695) */
int lp_bn_finalize2(const lp_fxsum* sums, float count0, float count1, int C, float eps, float momentum, float* mean, float* invstd,
                    float* running_mean, float* running_var, lp_stream_t stream);
/* y = [relu]((x - mean) * invstd * gamma + beta [+ residual]); relu_bits (optional, M*C/8 bytes): bit q of byte i = (y[8*i + q] > 0),
 * a 16x smaller ReLU mask for the backward pass */
int lp_bn_apply(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const void* residual,
                int relu, int M, int C, void* y, void* relu_bits, lp_stream_t stream);
/* both BatchNorm segments of a joint pass (lp_bn_fuse.seg_images) in ONE launch: rows [0, seg_rows) use row 0 of mean / invstd (2, C)
 * [and of sums (2, 2, C), with count0], the other rows use row 1 [count1] */
int lp_bn_apply_seg(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const void* residual,
                    int relu, int M, int C, int seg_rows, void* y, void* relu_bits, lp_stream_t stream);
/* The block-output pass of the optional "fp32 residual stream" policy (round 6; LP_RESIDUAL_FP32=1 in the engine - not the benchmarked default):
 * a block output o is kept as a bf16 pair, y = bf16(o) (what the convolutions read) and y_lo = bf16(o - y) (may be NULL: nobody adds this
 * output as an identity shortcut), and the residual added here is `residual` + `residual_lo` (the previous block's pair; residual_lo may be
 * NULL) or - `zd` given, residual / residual_lo NULL - the projection shortcut zd normalised in this pass and added unrounded.  Otherwise as
 * lp_bn_apply_seg / lp_bn_apply_seg_rbn.  (The reference keeps fp32 activations throughout: train.py:411-428.) */
int lp_bn_apply_seg_lo(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const void* residual,
                       const void* residual_lo, const void* zd, const float* mean_d, const float* invstd_d, const float* gamma_d,
                       const float* beta_d, int relu, int M, int C, int seg_rows, void* y, void* y_lo, void* relu_bits, lp_stream_t stream);
/* lp_bn_apply_seg whose residual is a PRE-normalisation tensor with its own BatchNorm (a block's projection shortcut, round 5): the shortcut is
 * normalised in the same pass - rounded to bf16 as its own lp_bn_apply would have stored it - instead of being written and read back.
 * Bit-identical to lp_bn_apply_seg(zd -> idt, no ReLU) followed by lp_bn_apply_seg(x, ..., residual = idt).
 * Reference: torchvision Bottleneck.forward (out = relu(bn3(conv3(.)) + downsample(x))) under models/base.py:398. */
int lp_bn_apply_seg_rbn(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const void* zd,
                        const float* mean_d, const float* invstd_d, const float* gamma_d, const float* beta_d, int relu, int M, int C,
                        int seg_rows, void* y, void* relu_bits, lp_stream_t stream);
/* sums (2,C) += [sum dz, sum dz*xhat], dz = dy masked by relu'(y_out) (y_out may be NULL) */
int lp_bn_bwd_reduce(const void* dy, const void* y_out, const void* x, const float* mean, const float* invstd, int M, int C,
                     lp_fxsum* sums, void* workspace, size_t workspace_bytes, lp_stream_t stream);
/* dx = gamma * invstd * (dz - sum(dz)/N - xhat * sum(dz*xhat)/N) [, dres = dz].  `sums`: the totals the two correction terms use - the
 * buffer after the SyncBatchNorm all-reduce, with count = rows x world size - or NULL: no batch-statistics terms (eval-mode BatchNorm is a
 * fixed affine map).  `sums_local` (this rank's sums, before any exchange; may equal sums) + dbeta_acc / dgamma_acc (optional): the
 * BatchNorm's parameter gradients d beta += sum dz, d gamma += sum dz*xhat over the segments, added by one thread per channel.
 * `terms_ws` (round 5): caller-owned scratch of segments x 2 x C floats, or NULL.  With it the call is two launches - a one-thread-per-value
 * conversion of the fixed-point sums to sum / count (+ the parameter gradients), then the streaming kernel reading plain floats; without it
 * one self-contained launch that converts the table into LDS per workgroup (C <= 2048 only; ~10 us slower per launch). */
int lp_bn_bwd_apply(const void* dy, const void* y_out, const void* x, const float* mean, const float* invstd, const float* gamma,
                    const lp_fxsum* sums, float count, int M, int C, void* dx, void* dres, const lp_fxsum* sums_local, float* dbeta_acc,
                    float* dgamma_acc, float* terms_ws, lp_stream_t stream);
int lp_bn_bwd_apply_seg(const void* dy, const void* y_out, const void* x, const float* mean, const float* invstd, const float* gamma,
                        const lp_fxsum* sums, float count0, float count1, int M, int C, int seg_rows, void* dx, void* dres,
                        const lp_fxsum* sums_local, float* dbeta_acc, float* dgamma_acc, float* terms_ws, lp_stream_t stream);
/* lp_bn_bwd_apply_seg for a block output whose masked gradient ALSO feeds the block's projection-shortcut BatchNorm (round 5): the same walk reads
 * that BatchNorm's pre-normalisation tensor zd and leaves its two backward reductions [sum dz, sum dz * xhat_d] per segment in sums_d
 * ([segments][2][C], added into) - what lp_bn_bwd_reduce(dres, NULL, zd, mean_d, invstd_d, ...) computes from one more pass over the gradient.
 * terms_ws is required; C / 8 must divide 256 (LP_ERR_UNSUPPORTED otherwise); workspace: lp_bn_bwd_ds_workspace_bytes(M, C).
 * Reference: autograd of bn3(z3) + downsample-bn(zd) -> relu under models/base.py:398 (torchvision Bottleneck.forward). */
size_t lp_bn_bwd_ds_workspace_bytes(int M, int C);
int lp_bn_bwd_apply_seg_ds(const void* dy, const void* y_out, const void* x, const float* mean, const float* invstd, const float* gamma,
                           const lp_fxsum* sums, float count0, float count1, int M, int C, int seg_rows, void* dx, void* dres,
                           const lp_fxsum* sums_local, float* dbeta_acc, float* dgamma_acc, float* terms_ws, const void* zd,
                           const float* mean_d, const float* invstd_d, lp_fxsum* sums_d, void* workspace, size_t workspace_bytes,
                           lp_stream_t stream);
/* 3x3 / stride 2 / pad 1; argmax_u8 (B,Ho,Wo,C) records the winning tap (first maximum, ATen tie rule) for the backward gather */
int lp_maxpool_fwd(const void* x, int B, int Hi, int Wi, int C, void* y, void* argmax_u8, lp_stream_t stream);
int lp_maxpool_bwd(const void* argmax_u8, const void* dy, int B, int Hi, int Wi, int C, void* dx, lp_stream_t stream);
/* Stem: BatchNorm + ReLU + MaxPool2d(3, 2, 1) without ever storing the activation between them (torchvision resnet50 children
 * bn1, relu, maxpool; reference models/backbones/factory.py:322-348).  Forward = lp_bn_apply(relu) -> lp_maxpool_fwd, bit for bit
 * (each tap is rounded to bf16 as lp_bn_apply would have stored it).  Backward: the activation's gradient is rebuilt on the fly from
 * the pooled gradient dy, the arg-max bytes and z (ReLU gate recomputed from z): lp_bn_pool_bwd_reduce leaves [sum g, sum g * xhat]
 * in sums[2][C] (fixed point), lp_bn_pool_bwd_apply writes d z (and adds the sums into d beta / d gamma, as lp_bn_bwd_apply does). */
int lp_bn_relu_maxpool_fwd(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta, int B, int Hi, int Wi,
                           int C, void* y, void* argmax_u8, lp_stream_t stream);
int lp_bn_pool_bwd_reduce(const void* argmax_u8, const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, int B, int Hi, int Wi, int C, lp_fxsum* sums, lp_stream_t stream);
int lp_bn_pool_bwd_apply(const void* argmax_u8, const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, const lp_fxsum* sums, float count, int B, int Hi, int Wi, int C, void* dx,
                         const lp_fxsum* sums_local, float* dbeta_acc, float* dgamma_acc, lp_stream_t stream);
int lp_images_to_nhwc4(const float* images_nchw, int B, int H, int W, void* out_bf16, lp_stream_t stream);
/* (B,h,w,4*c_out) -> (B,2h,2w,c_out) stored with channel pitch ld >= c_out (pad channels untouched); inverse = 1 maps the
 * gradient (pitch ld) back */
int lp_pixel_shuffle(const void* in, int B, int h, int w, int c_out, int ld, int inverse, void* out, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * ViT-S/16 backbone glue (models/backbones/vit.py:16-49 -> transformers ViTModel; backbone = "vits_dino",
 * models/backbones/factory.py:188-190).  The Linear layers and attention products run on lp_gemm_nt / lp_conv_wgrad.
 * Residual stream and statistics fp32, GEMM operands bf16.
 * ------------------------------------------------------------------------------------------------------ */
/* (B,3,H,W) fp32 -> [B*(H/P)*(W/P)][3*P*P] bf16 patch rows, k = (c, ky, kx) (= Conv2d weight.flatten(1)) */
int lp_vit_patchify(const float* images_nchw, int B, int H, int W, int patch, void* out_bf16, lp_stream_t stream);
/* x[b][0] = cls + pos[0], x[b][1+p] = patch[b][p] + pos[1+p]  (pos already interpolated, (1+Np, D) fp32) */
int lp_vit_tokens_fwd(const void* patch_bf16, const float* cls, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream);
/* dpatch = bf16(dx[:, 1:]);  dpos[t] = sum_b dx[b][t]  (d cls = dpos[0]) */
int lp_vit_tokens_bwd(const float* dx, int B, int Np, int D, void* dpatch_bf16, float* dpos, lp_stream_t stream);
/* Token assembly of the multi-view transformer tracker (models/heatmap_tracker_multiview.py:143-223 forward_vit: ViTEmbeddings(...)[:, 1:]
 * + view_embeddings[v], reshaped to (B, V*Np, D)): no [CLS] row; row (b*V + v)*Np + p of `patch` becomes token v*Np + p of sample b.
 *   x[b][v*Np + p][:] = (patch[(b*V + v)*Np + p][:] + pos[1 + p][:]) + view[v][:]      - fp32, the two additions in THIS order
 * pos: the interpolated (1 + Np, D) table (row 0, the [CLS] position, is not read); view (V, D).  D must be a multiple of 64
 * (LP_ERR_UNSUPPORTED otherwise). */
int lp_vit_mv_tokens_fwd(const void* patch_bf16, const float* pos, const float* view, int B, int V, int Np, int D, float* x,
                         lp_stream_t stream);
/* Backward, one pass over dx (B*V*Np, D): dpatch = bf16(dx) (round to nearest even; same row order),
 * dpos (1 + Np, D): dpos[0] = 0, dpos[1 + p] = sum_{b,v} dx;  dview (V, D): dview[v] = sum_{b,p} dx.  All three are WRITTEN, not
 * accumulated.  The sums are a two-level reduction in a fixed order (workgroup partials in `workspace`, combined by a second small
 * launch; no floating-point atomics): the same input gives the same bits.  workspace: lp_vit_mv_tokens_bwd_workspace_bytes(B, V, Np, D)
 * bytes (0 for an unsupported shape), contents undefined before and after.  D must be a multiple of 64 and V * ceil(B / group) <= 65535
 * (LP_ERR_UNSUPPORTED); a null pointer, a non-positive dimension or a workspace that is too small: LP_ERR_ARGUMENT. */
size_t lp_vit_mv_tokens_bwd_workspace_bytes(int B, int V, int Np, int D);
int lp_vit_mv_tokens_bwd(const float* dx, int B, int V, int Np, int D, void* dpatch_bf16, float* dpos, float* dview, void* workspace,
                         size_t workspace_bytes, lp_stream_t stream);
/* ---- camera geometry of the calibrated multi-view losses (csrc/cameras.hip; reference data/cameras.py, data/bboxes.py:194-219,
 * losses/losses.py:999-1126).  All fp32.  points (B, V, K, 2) frame px; intrinsics (B, V, 3, 3); extrinsics (B, V, 3, 4); dist12 (B, V, 12):
 * OpenCV order k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, shorter sets padded with zeros by the caller; bbox (B, 4 V) [x, y, h, w] per view or
 * NULL.  P = V (V - 1) / 2 camera pairs in itertools.combinations order.  V <= LP_CAM_MAX_VIEWS (LP_ERR_UNSUPPORTED otherwise).
 *   undistort   x0 = (u - cx) / fx, y0 = (v - cy) / fy; 5 fixed-point iterations of x = (x0 - dx(x, y)) * inv(x, y)
 *   triangulate h = right singular vector of the smallest singular value of the 4 x 4 DLT matrix; X = h[:3] / h[3] (|h[3]| > 1e-8, else h[:3]);
 *               a keypoint that is NaN in either view gives NaN for that (pair, keypoint) and takes no gradient
 *   project     Xc = R X + t; (x, y) = Xc[:2] / Xc[2] (same guard); the distortion model forward; u = fx x + cx, v = fy y + cy;
 *               with bbox: u = (u - bx) / bw * model_w, v = (v - by) / bh * model_h
 * lp_cam_chain_fwd: p3d (B, P, K, 3) = every pair's triangulation; p2d (B, V, K, 2) (may be NULL: triangulation only) = the mean of the pairs
 * (one NaN pair makes it NaN) projected into every view.  ONE launch, one workgroup per sample.
 * lp_cam_chain_bwd: gpoints (B, V, K, 2) = d / d points of (g3d . p3d + g2d . p2d); g3d or g2d may be NULL (not both); p3d (the forward's
 * output) is required with g2d.  Written, not accumulated; 0 for a NaN point; a NaN mean passes no gradient from g2d.  ONE launch; sums in a
 * fixed order, no atomics: the same input gives the same bits.  workspace: lp_cam_chain_workspace_bytes(B, V, K) bytes (0 for an
 * unsupported shape), contents undefined before and after. */
#define LP_CAM_MAX_VIEWS 32
size_t lp_cam_chain_workspace_bytes(int B, int V, int K);
int lp_cam_chain_fwd(const float* points, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox, float model_h,
                     float model_w, int B, int V, int K, float* p3d, float* p2d, lp_stream_t stream);
int lp_cam_chain_bwd(const float* points, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox, float model_h,
                     float model_w, int B, int V, int K, const float* p3d, const float* g3d, const float* g2d, void* workspace,
                     size_t workspace_bytes, float* gpoints, lp_stream_t stream);
/* stand-alone projection of points_3d (B, K, 3) into every view -> p2d (B, V, K, 2), and its backward g3d (B, K, 3) = sum over the views (in
 * order) of the projection's transpose applied to g2d; 0 for a NaN point */
int lp_cam_project_fwd(const float* points_3d, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                       float model_h, float model_w, int B, int V, int K, float* p2d, lp_stream_t stream);
int lp_cam_project_bwd(const float* points_3d, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                       float model_h, float model_w, int B, int V, int K, const float* g2d, float* g3d, lp_stream_t stream);
/* loss = mean over the valid (b, p, k) of ||targ_3d[b, k] - pred_3d[b, p, k]||_2 (invalid: a NaN in either; 0 if none is valid);
 * grad_unit (B, P, K, 3) = d loss / d pred_3d for upstream 1 (0 where invalid or where the distance is exactly 0).  One launch. */
int lp_cam_pairwise_fwd_bwd(const float* targ_3d, const float* pred_3d, int B, int P, int K, float* loss, float* grad_unit, lp_stream_t stream);
/* y (R,D) (+)= w (R,Q) @ x (Q,D), or with transpose_w: y (Q,D) (+)= w^T @ x (R,D): bicubic position-embedding interpolation */
int lp_small_matmul(const float* w, const float* x, int R, int Q, int D, int transpose_w, int accumulate, float* y, lp_stream_t stream);
/* x_out = x (+ delta_bf16);  y = LayerNorm(x_out) in bf16;  drop_T > 0: rows with row % drop_T == 0 ([CLS]) are dropped from y and
 * the rest compacted (the (B, h, w, D) feature map).  x_out may alias x; mean / rstd (M,) are kept for the backward pass.
 * x_out is required with a delta and optional without one: a non-NULL x_out then receives a copy of x.  (The fp32 form
 * lp_f32_layernorm_fwd differs there: without a delta it never writes x_out.) */
int lp_layernorm_fwd(const float* x, const void* delta_bf16, float* x_out, const float* gamma, const float* beta, float eps, int M,
                     int D, int drop_T, void* y_bf16, float* mean, float* rstd, lp_stream_t stream);
/* dx_acc += LayerNorm backward of dy (bf16, same row mapping as y);  dgamma_acc / dbeta_acc accumulate too.  A row that drop_T leaves
 * without a dy takes dy = 0: its dx_acc stays bit for bit, and in the two forms below its dx_bf16 is the cast of that value and it is
 * part of the column sums (as the LayerScale forms further down say of their own dropped rows). */
int lp_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, int M, int D,
                     int drop_T, float* dx_acc, float* dgamma_acc, float* dbeta_acc, lp_stream_t stream);
/* same, and the updated dx_acc is also written rounded to bf16 (what the next Linear layer's backward reads; the LayerNorms are
 * those of transformers ViTLayer / ViTModel.layernorm behind reference models/backbones/vit.py:26-27) */
int lp_layernorm_bwd_bf16(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, int M, int D,
                          int drop_T, float* dx_acc, void* dx_bf16, float* dgamma_acc, float* dbeta_acc, lp_stream_t stream);
int lp_gelu_fwd(const void* x_bf16, size_t n, void* y_bf16, lp_stream_t stream);                       /* exact (erf) GELU */
int lp_gelu_bwd(const void* x_bf16, const void* dy_bf16, size_t n, void* dx_bf16, lp_stream_t stream);
/* The two producers of a Linear layer's dy in the ViT backward, leaving that layer's BIAS gradient (the column sums of the bf16 tensor they
 * write, accumulated into colsum_acc) on the way: the weight gradient then needs no bias pass (lp_conv_wgrad instead of lp_conv_wgrad_bias). */
int lp_gelu_bwd_colsum(const void* x_bf16, const void* dy_bf16, int rows, int cols, void* dx_bf16, float* colsum_acc, lp_stream_t stream);
int lp_layernorm_bwd_bf16_colsum(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, int M, int D,
                                 int drop_T, float* dx_acc, void* dx_bf16, float* dgamma_acc, float* dbeta_acc, float* colsum_acc,
                                 lp_stream_t stream);
/* LayerScale (transformers Dinov2LayerScale: a learned per-channel factor on each branch output, in front of the residual add) inside the
 * two LayerNorm walks that already touch those tensors - the DINOv2 backbones ("vits_dinov2" / "vitb_dinov2").
 * forward: lp_layernorm_fwd with x_out = x + (float(delta_bf16) * ls[D]) - an fp32 product, then an fp32 sum: two roundings in that order,
 *   never one fused multiply-add - and the LayerNorm of x_out as there (delta_bf16, ls and x_out are required).
 * backward: lp_layernorm_bwd_bf16_colsum for a stream gradient that is consumed through a LayerScale: with o the updated dx_acc,
 *   dx_bf16 = bf16(ls o o) (round to nearest even), colsum_acc[D] += sum_rows ls o o (of the fp32 products; NULL: not taken),
 *   dls_acc[D] += sum_rows o o float(branch_bf16) - `ls` and `branch_bf16` (M, D) are the scale and the unscaled forward output (the `delta`
 *   the forward read) of the branch that CONSUMES the emitted gradient.  dx_acc / dgamma_acc / dbeta_acc exactly as lp_layernorm_bwd; rows
 *   without a dy (drop_T) still carry stream gradient and contribute to all three sums. */
int lp_layernorm_ls_fwd(const float* x, const void* delta_bf16, const float* ls, float* x_out, const float* gamma, const float* beta, float eps,
                        int M, int D, int drop_T, void* y_bf16, float* mean, float* rstd, lp_stream_t stream);
int lp_layernorm_ls_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, const float* ls,
                        const void* branch_bf16, int M, int D, int drop_T, float* dx_acc, void* dx_bf16, float* dgamma_acc, float* dbeta_acc,
                        float* colsum_acc, float* dls_acc, lp_stream_t stream);
/* The DINOv3 backbones ("vits_dinov3" / "vitb_dinov3", transformers DINOv3ViTModel): csrc/rope.hip and two more forms of the walks above.
 *
 * lp_layernorm_ls_fwd_px / _bwd_px: lp_layernorm_ls_fwd / _bwd with the `n_prefix` leading rows of every drop_T rows ([CLS] and the register
 *   tokens) dropped from y / carrying no dy, instead of row 0 alone: y holds the (M / drop_T) * (drop_T - n_prefix) kept rows in order
 *   (0 <= n_prefix <= drop_T; drop_T = 0: nothing dropped).  The same kernels: n_prefix = 1 gives the bits of the forms above.  Dropped rows
 *   still carry stream gradient and contribute to dgamma / dbeta (with a zero dy) / colsum / dls.
 *
 * lp_rope_fwd / _bwd: the rotary position embedding on the Q and K columns of the fused token rows qkv[(b * T + t) * ld + ...] (Q of head h at
 *   column h * 64, K at k_off + h * 64), IN PLACE, for the rows t >= n_prefix of each of the B sequences of T tokens; the prefix rows, the V
 *   columns and everything else in the row are neither read nor written.  `table` is (n_tab, T - n_prefix, 64) fp32: per patch token
 *   cos[0:32] | sin[0:32] (the 32 distinct columns of the head's 64); sequence b uses table tab_of_seq[b] (a device int32 array; NULL: table 0
 *   for all; an index outside [0, n_tab) is clamped), so a joint pass of two batches with their own coordinate draws is one launch.
 *   forward, for d < 32: out[d] = x[d] cos[d] - x[d + 32] sin[d],  out[d + 32] = x[d + 32] cos[d] + x[d] sin[d] - in fp32, two products and
 *   one sum / difference (never a fused multiply-add), one rounding to bf16 (nearest even).  backward: the transposed rotation (sin -> -sin)
 *   of dQ / dK.  No LDS, no atomics: two runs give the same bits.  LP_ERR_UNSUPPORTED: head_dim != 64, or ld / k_off / a base pointer that
 *   breaks 16-byte alignment; LP_ERR_ARGUMENT: null qkv / table, non-positive sizes, n_prefix outside [0, T], Q / K blocks outside the row.
 *
 * lp_vit_reg_tokens_fwd / _bwd: the token assembly with R >= 0 register tokens and no position table (D % 8 == 0):
 *   x[b][0] = cls,  x[b][1 + r] = reg[r],  x[b][1 + R + p] = float(patch[b * Np + p]);  backward: dpatch = bf16(dx[:, 1 + R:]),
 *   dcls = sum_b dx[b][0], dreg[r] = sum_b dx[b][1 + r] - images in ascending order, no atomics, WRITTEN (not accumulated), as
 *   lp_vit_mv_tokens_bwd does.  reg / dreg may be NULL when R = 0. */
int lp_layernorm_ls_fwd_px(const float* x, const void* delta_bf16, const float* ls, float* x_out, const float* gamma, const float* beta,
                           float eps, int M, int D, int drop_T, int n_prefix, void* y_bf16, float* mean, float* rstd, lp_stream_t stream);
int lp_layernorm_ls_bwd_px(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, const float* ls,
                           const void* branch_bf16, int M, int D, int drop_T, int n_prefix, float* dx_acc, void* dx_bf16, float* dgamma_acc,
                           float* dbeta_acc, float* colsum_acc, float* dls_acc, lp_stream_t stream);
int lp_rope_fwd(void* qkv_bf16, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh,
                int head_dim, lp_stream_t stream);
int lp_rope_bwd(void* dqkv_bf16, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh,
                int head_dim, lp_stream_t stream);
int lp_vit_reg_tokens_fwd(const void* patch_bf16, const float* cls, const float* reg, int B, int R, int Np, int D, float* x, lp_stream_t stream);
int lp_vit_reg_tokens_bwd(const float* dx, int B, int R, int Np, int D, void* dpatch_bf16, float* dcls, float* dreg, lp_stream_t stream);
/* The SAM backbone ("vitb_sam", transformers SamVisionEncoder with relative positions off and without its neck): csrc/window.hip.
 *
 * Window layers attend inside ws x ws windows of the (gh, gw) token grid, zero-padded on the bottom and right to nWy * ws x nWx * ws
 * (nWy = ceil(gh / ws), nWx = ceil(gw / ws), nW = nWy * nWx).  Window b * nW + wy * nWx + wx holds, as its token ty * ws + tx, the grid
 * position (wy * ws + ty, wx * ws + tx) of image b; a position outside the grid is a pad row.  The attention entry points then run
 * unchanged on B * nW sequences of ws * ws tokens.
 *
 * lp_window_partition: dst[(B * nW * ws * ws)][cols] (dense) gathered from src[(b * gh + gy) * gw + gx][...] (rows ld_src elements apart,
 *   ld_src >= cols).  Pad rows are copies of fill[cols] - for the fused qkv tensor: the qkv bias as the GEMM's store pass rounds it, because a
 *   padded token is zero after the LayerNorm and still takes part in its window's soft-max - or zeros when fill is NULL (gradients).
 * lp_window_unpartition: the inverse move, dst[(b * gh + gy) * gw + gx][0 .. cols) (rows ld_dst apart; columns behind cols untouched) from the
 *   dense window rows; pad rows are dropped.  With pad_colsum_acc != NULL, pad_colsum_acc[c] += sum over ALL pad rows of src[.][c], in fp32:
 *   the pad rows' dK / dV are gradient of the qkv bias.  ADDED to what the vector holds, once per call (with no pad rows it is left
 *   untouched), in an order fixed by the shapes alone - 64 row slots take the pad positions 64 apart in ascending order, then the slots are
 *   added in ascending order - with no atomics: the same inputs give the same bits.
 * Both are moves of 16-byte pieces: every bit pattern (NaN payloads, -0.0) arrives unchanged; one launch each, nothing read back.
 * LP_ERR_ARGUMENT: a null src / dst, a non-positive size, ws < 1, a pitch below cols - nothing is written.  LP_ERR_UNSUPPORTED: cols or the
 * pitch not a multiple of 16 bytes, or src / dst / fill not 16-byte aligned.
 *
 * lp_vit_pos_tokens_fwd / _bwd: tokens without a prefix row, x[b][p] = float(patch[b * Np + p]) + pos[p] (pos (Np, D) fp32, D % 8 == 0);
 *   backward: dpatch = bf16(dx), dpos[p] = sum_b dx[b][p] - images in ascending order, WRITTEN (not accumulated), as lp_vit_reg_tokens_bwd.
 * lp_resid_out_fwd / _bwd: the residual add behind the last layer of a model without a final LayerNorm, x_out = x + float(delta) (x_out may be
 *   x) and y = bf16(x_out), the features the head reads (n elements, n % 8 == 0);  backward: dx = float(dy), WRITTEN - the stream gradient
 *   starts as the head's gradient. */
int lp_window_partition(const void* src_bf16, int ld_src, int B, int gh, int gw, int ws, int cols, const void* fill_bf16, void* dst_bf16,
                        lp_stream_t stream);
int lp_window_unpartition(const void* src_bf16, int B, int gh, int gw, int ws, int cols, void* dst_bf16, int ld_dst, float* pad_colsum_acc,
                          lp_stream_t stream);
int lp_vit_pos_tokens_fwd(const void* patch_bf16, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream);
int lp_vit_pos_tokens_bwd(const float* dx, int B, int Np, int D, void* dpatch_bf16, float* dpos, lp_stream_t stream);
int lp_resid_out_fwd(const float* x, const void* delta_bf16, size_t n, float* x_out, void* y_bf16, lp_stream_t stream);
int lp_resid_out_bwd(const void* dy_bf16, size_t n, float* dx, lp_stream_t stream);
/* in place: s[r][:n] = softmax(scale * s[r][:n]), s[r][n:ld] = 0   /   dp <- scale * p * (dp - sum(dp * p)) */
int lp_softmax_rows_fwd(void* s_bf16, int rows, int n, int ld, float scale, lp_stream_t stream);
int lp_softmax_rows_bwd(const void* p_bf16, void* dp_bf16, int rows, int n, int ld, float scale, lp_stream_t stream);
/* out[z][c][r] = in[z][r][c] (r < R, c < Cc), out[z][c][R:ldo] = 0;  z = (zb, zh) with element strides */
int lp_transpose_batched(const void* in_bf16, int R, int Cc, int ldi, long long in_b, long long in_h, void* out_bf16, int ldo,
                         long long out_b, long long out_h, int nb, int nh, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Batch producers: what sits directly BEFORE the step.
 *   lp_frames_resize / lp_frames_augment   the device half of data/video/dali.py:135-192 video_pipe after the decoder:
 *        fn.resize -> [fn.warp_affine(matrix, fill_value=0, inverse_map=False) -> fn.brightness_contrast -> fn.noise.shot]
 *        -> /255 -> fn.crop_mirror_normalize(mean, std, output_layout="FCHW"); the (2,3) matrix is the `transforms` entry of
 *        UnlabeledBatchDict (data/video/dali.py:267-330) that lp_decode_fwd's frame map undoes.  DALI is not vendored:
 *        its published operator definitions are restated (oracle/restated.py), parity unpinned.
 *   lp_labeled_keypoints                   data/datasets.py:262-376 (imgaug Resize keypoint projection, hflip + left/right
 *        swap), :465-472 (visibility synthesised from NaN labels), :496-508 (out-of-frame keypoints become NaN); feed the
 *        result to lp_heatmap_gen for HeatmapDataset.compute_heatmap's targets.
 * ------------------------------------------------------------------------------------------------------ */
enum { LP_BORDER_RENORM = 0, /* filter window cut at the image edge and renormalised (PIL / torch antialias)       */
       LP_BORDER_CLAMP = 1   /* edge pixels replicated under the full window (DALI resampling)                     */ };

typedef struct lp_frame_norm {
    float mean[3], std[3]; /* per channel, in [0,1] units (ImageNet statistics in the reference, data/__init__.py:46-47) */
} lp_frame_norm;

typedef struct lp_frame_augment {
    int has_matrix;
    float matrix[6];        /* row-major (2,3), maps SOURCE to DESTINATION pixel-centre coordinates (inverse_map=False)   */
    float brightness, contrast, contrast_center; /* out = brightness * (center + contrast * (in - center)); DALI: 0.5 for float input */
    float shot_factor;      /* out = Poisson(max(in,0) / factor) * factor on the [0,255] scale; 0 = off                   */
    unsigned long long seed; /* counter-based generator: the noise depends only on (seed, frame, pixel, channel)         */
} lp_frame_augment;

/* src u8 (S, Hs, Ws, 3) with byte strides -> antialiased linear resize to (H, W).  finish_norm == NULL: dst = fp32 (S,H,W,3) in
 * [0,255] (input of lp_frames_augment); else dst = fp32 (S,3,H,W) = (v/255 - mean) / std (imgaug="default": no augmentation) */
int lp_frames_resize(const void* src_u8, int S, int Hs, int Ws, long long frame_stride, int row_stride, int H, int W, int border,
                     const lp_frame_norm* finish_norm, float* dst, lp_stream_t stream);
/* Same layouts, bicubic interpolation without antialiasing (Keys kernel, A = -0.75, half-pixel centres, taps clamped): imgaug
 * iaa.Resize's default (OpenCV INTER_CUBIC), the last imgaug step of every LABELED image (data/datasets.py:137-143).  round_u8 != 0:
 * the interpolated value is rounded and saturated to [0, 255] first - imgaug returns uint8 images. */
int lp_frames_resize_cubic(const void* src_u8, int S, int Hs, int Ws, long long frame_stride, int row_stride, int H, int W, int round_u8,
                           const lp_frame_norm* finish_norm, float* dst, lp_stream_t stream);
/* src fp32 (S,H,W,3) in [0,255] -> dst fp32 (S,3,H,W); one parameter set per call = per DALI sample (a whole sequence) */
int lp_frames_augment(const float* src_hwc, int S, int H, int W, const lp_frame_augment* aug, const lp_frame_norm* norm,
                      float* dst_nchw, lp_stream_t stream);
/* kp_src (B,K,2) source px, src_hw (B,2) = source (height, width); optional affine (B,2,3) on source px, hflip (B) 0/1 with the
 * keypoint permutation swap (K), vis_in (B,K) 0/1/2 (NULL: synthesised from NaN labels, NaN -> uniform_heatmaps ? 1 : 0, else 2).
 * kp_out (B,K,2) model px with out-of-frame points set to NaN, vis_out (B,K).  kp_out must not alias kp_src. */
int lp_labeled_keypoints(const float* kp_src, const float* src_hw, const float* affine, const int* hflip, const int* swap,
                         const int* vis_in, int uniform_heatmaps, int B, int K, int H, int W, float* kp_out, int* vis_out,
                         lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Crop-zoom prediction (csrc/cropzoom.hip; reference utils/cropzoom.py): a detector's keypoints -> one box per frame -> [rolling median] ->
 * each frame's own region of interest resampled from the uint8 frame into the pose model's input planes.  The boxes stay in device memory
 * from the first call to the last; no call reads anything back.
 * ------------------------------------------------------------------------------------------------------ */
enum { LP_BBOX_MAX_ANCHORS = 64,        /* anchor indices travel as kernel arguments (bytes: K <= 256 when a list is given)          */
       LP_BBOX_SMOOTH_MAX_WINDOW = 255  /* the median is found by counting ranks: window^2 comparisons per frame and column        */ };

/* keypoints (N, K, 2) fp32 frame px -> bbox (N, 4) int32 [x, y, h, w]: _compute_bbox_df / _calculate_bbox_size (utils/cropzoom.py:31-143) in
 * double precision with the sums taken in keypoint order.  `anchors` is a HOST array of n_anchors keypoint indices (0: every keypoint).
 * Ratio mode (crop_ratio > 0, crop_height = crop_width = 0): size = ceil(max(x span, y span) * crop_ratio), made even, h = w = size.
 * Fixed mode (crop_height, crop_width > 0, crop_ratio = 0): h = crop_height + crop_height % 2, w likewise.
 * Corner = trunc(centroid - [h / 2, w / 2]) toward zero - (sic) x moves by half the HEIGHT, as in the reference, so box files interchange.
 * Deviation: a frame with a non-finite anchor coordinate or a size of 0 gets [0, 0, 0, 0] (the reference crashes later on such a frame). */
int lp_bbox_from_keypoints(const float* keypoints, int N, int K, const int* anchors, int n_anchors, double crop_ratio, int crop_height,
                           int crop_width, int* bbox, lp_stream_t stream);
/* DataFrame.rolling(window, center=True, min_periods=1).median().round(0).astype(int) per column (utils/cropzoom.py:391-392): frame i sees
 * frames [i - window / 2, i + (window - 1) / 2] cut to [0, N); an even count gives the mean of the two middle values, rounded half to even.
 * window > LP_BBOX_SMOOTH_MAX_WINDOW: LP_ERR_UNSUPPORTED.  bbox_out must not alias bbox_in. */
int lp_bbox_smooth(const int* bbox_in, int N, int window, int* bbox_out, lp_stream_t stream);
/* src u8 (S, Hs, Ws, 3) with byte strides, bbox (S, 4) int32 [x, y, h, w] ON THE DEVICE -> dst fp32 (S, 3, H, W) = (v / 255 - mean) / std.
 * Frame s is the virtual h_s x w_s image whose pixel (i, j) is src[s][y_s + i][x_s + j] inside the frame and 0 outside it (zero padding);
 * it is resampled to (H, W) by lp_frames_resize's rule (triangle filter of radius max(1, scale) per axis, `border` applied at the edge of
 * the virtual image) with a scale of its own.  The result is bit-identical to lp_frames_resize of the materialised crop.  A box with
 * h <= 0 or w <= 0 (or a side above 65536) gives the normalised black frame. */
int lp_frames_crop_resize(const void* src_u8, int S, int Hs, int Ws, long long frame_stride, int row_stride, const int* bbox, int H, int W,
                          int border, const lp_frame_norm* norm, float* dst, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Labeled-frame augmentation (csrc/labelaug.hip): the imgaug "dlc" presets of data/augmentations.py:122-238, restated from imgaug's
 * documented operator definitions (imgaug and OpenCV are not vendored: pixel parity with imgaug itself is UNPINNED).
 * Every entry point is ONE launch sequence for the whole batch: `params` is a device array of B lp_labelaug_image (drawn on the host),
 * an image whose flag for a stage is off is copied through.  u8 images are contiguous (B, H, W, 3); every stage rounds and saturates to
 * uint8 as imgaug does between augmenters.  Continuous coordinates put the centre of pixel (i, j) at (j + 0.5, i + 0.5).
 * Per-pixel randomness is Philox4x32-10 keyed by `seed` and counters (cell or pixel index, image_id | op << 16 | channel << 20 | what << 24):
 * a value never depends on the launch geometry.
 * ------------------------------------------------------------------------------------------------------ */
enum { LP_AUG_GEOM = 1, LP_AUG_BLUR = 2, LP_AUG_DROPOUT = 4, LP_AUG_DROP_PER_CHANNEL = 8, LP_AUG_SALT = 16, LP_AUG_PEPPER = 32,
       LP_AUG_ELASTIC = 64, LP_AUG_HISTEQ = 128, LP_AUG_CLAHE = 256, LP_AUG_EMBOSS = 512, LP_AUG_CROPPAD = 1024, LP_AUG_HFLIP = 2048 };
enum { LP_AUG_OP_DROPOUT = 0, LP_AUG_OP_SALT = 1, LP_AUG_OP_PEPPER = 2, LP_AUG_OP_ELASTIC = 3 };   /* the `op` of the Philox counter */
enum { LP_AUG_LOCAL_BLUR_COARSE = 0, LP_AUG_LOCAL_EMBOSS = 1 };
#define LP_AUG_ELASTIC_MAX_RADIUS 20

typedef struct lp_labelaug_image {   /* 60 four-byte words, no padding */
    int flags;
    int image_id;           /* the image's number in the Philox counters (its index in the batch it was drawn for; < 65536)              */
    float geom[6];          /* LP_AUG_GEOM: row-major (2,3) DESTINATION -> SOURCE map of Rot90 then Affine on continuous coordinates      */
    float blur[25];         /* LP_AUG_BLUR: 5 x 5 correlation weights (MotionBlur's rotated line, sum 1), border reflect-101             */
    float emboss[9];        /* LP_AUG_EMBOSS: 3 x 3 correlation weights, (1 - alpha) identity + alpha emboss(strength)                    */
    int coarse_gh[3], coarse_gw[3];  /* grid of CoarseDropout / CoarseSalt / CoarsePepper; pixel (y, x) lies in cell (y gh / H, x gw / W)  */
    unsigned coarse_thr[3]; /* a cell is masked when (Philox word >> 8) < thr, thr = p 2^24                                              */
    float elastic_alpha;    /* LP_AUG_ELASTIC: displacement = alpha * Gaussian-filtered U(-1, 1) noise                                    */
    int clahe_clip, clahe_tiles_y, clahe_tiles_x, clahe_slot; /* clip count per bin (>= 1), tile grid, index into the look-up-table buffer */
    int pad[4];             /* LP_AUG_CROPPAD: top, right, bottom, left in px; positive pads with zeros, negative crops                  */
} lp_labelaug_image;

/* Rot90 and Affine as one inverse-mapped bilinear gather with zero fill */
int lp_labelaug_geom(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, void* dst_u8, lp_stream_t stream);
/* which = LP_AUG_LOCAL_BLUR_COARSE: MotionBlur -> CoarseDropout -> CoarseSalt -> CoarsePepper;  LP_AUG_LOCAL_EMBOSS: Emboss.  One stencil
 * pass over an LDS tile with a 2-pixel halo; the coarse masks are evaluated per pixel from the cell index.  salt_lut: 256 bytes, the
 * quantile table of the salt value (pepper = 255 - salt), indexed by the top byte of the pixel's Philox word. */
int lp_labelaug_local(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, int which, const void* salt_lut,
                      unsigned long long seed, void* dst_u8, lp_stream_t stream);
/* field fp32 (B, 2, H, W) = (dx, dy) = alpha * G_sigma * U(-1, 1) for the images with LP_AUG_ELASTIC (others: not written); the Gaussian is
 * cut at 4 sigma (<= LP_AUG_ELASTIC_MAX_RADIUS taps each side), border reflect-101; tmp: workspace of the same size */
int lp_labelaug_elastic_field(int B, int H, int W, const lp_labelaug_image* params, float sigma, unsigned long long seed, float* tmp,
                              float* field, lp_stream_t stream);
/* dst(x, y) = bicubic (Keys, A = -0.75) sample of src at (x + dx, y + dy), taps outside the image read 0 */
int lp_labelaug_elastic_apply(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, const float* field, void* dst_u8,
                              lp_stream_t stream);
/* 256-bin equalisation per channel: lut[v] = round(255 (cdf[v] - cdf_min) / (n - cdf_min)) in integers.  ws: B*3*256 unsigned (zeroed
 * here); lut_out: B*3*256 bytes (written for the images with LP_AUG_HISTEQ) */
int lp_labelaug_histeq(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, unsigned* ws, void* lut_out, void* dst_u8,
                       lp_stream_t stream);
/* CLAHE per channel: tiles of ceil(H / tiles_y) x ceil(W / tiles_x) px over the image extended by reflection-101, histogram clipped at
 * clahe_clip with the excess redistributed, lut = round(255 cdf / area) in integers, bilinear blend of the four nearest tiles' tables.
 * slot_image (n_slots): image index of each look-up-table slot; luts: n_slots * max_ty * max_tx * 3 * 256 bytes */
int lp_labelaug_clahe(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, const int* slot_image, int n_slots,
                      int max_ty, int max_tx, void* luts, void* dst_u8, lp_stream_t stream);
/* CropAndPad (keep_size=False) -> cubic Resize to (H, W) (lp_frames_resize_cubic's arithmetic on the cropped / zero-padded image) ->
 * /255 -> normalise -> optional mirrored write (LP_AUG_HFLIP): fp32 (B, 3, H, W) */
int lp_labelaug_finish(const void* src_u8, int B, int Hs, int Ws, const lp_labelaug_image* params, int H, int W, const lp_frame_norm* norm,
                       float* dst, lp_stream_t stream);
/* kp (B,K,2) source px -> affine (B,2,3) (NULL: identity) -> minus the displacement sampled (bilinear) at the moved point for images with
 * LP_AUG_ELASTIC when field != NULL (first-order inverse of the elastic map).  NaN stays NaN.  kp_out must not alias kp. */
int lp_labelaug_keypoints(const float* kp, int B, int K, const float* affine, const lp_labelaug_image* params, const float* field, int H,
                          int W, float* kp_out, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Patch masking (csrc/patchmask.hip): the multi-view transformer's masking curriculum (callbacks.py:279-401, PatchMasker) - choose
 * `count` patches per image and zero them, ONE launch for the batch, no workspace, nothing read back.
 * images / out: fp32 (BV, C, H, W) contiguous, BV = samples x views.  Patch grid nh = H / patch, nw = W / patch (floor), N = nh nw; patch p
 * covers rows (p / nw) patch ... and columns (p % nw) patch ...; pixels beyond nh patch / nw patch are never masked.
 * mask_in == NULL: word(i, p) = the first output word of Philox4x32-10 with key `key` and counter (p, i, 0, 0); patch p of image i is masked
 *   iff its rank among the N pairs (word, p) in ascending lexicographic order is < count: exactly `count` patches per image for any N, a
 *   function of (key, i, p) only - never of the launch geometry.  The caller packs key = (seed mod 2^32) | (step mod 2^32) << 32.  Unlike the
 *   reference's generator seed (patch_seed + step + 1000 b + 100 v, which step 100 of sample 0 shares with step 0 of view 1), two different
 *   (step, sample, view) never share a stream.
 * mask_in != NULL: (BV, N) fp32, 0 = mask, anything else = keep; used as given, `count` is ignored.
 * mask_out (BV, N): 1.0f (kept) or 0.0f (masked).  out: every pixel of a masked patch, in all C channels, is +0.0f whatever it held (NaN and
 * Inf included); every other pixel is copied bit for bit (NaN payloads, -0.0).  out == images (in place) is allowed and gives the same
 * bits; any other overlap is not.  `images` is otherwise not written.
 * LP_ERR_UNSUPPORTED: N > 1024 (512 x 512 at patch 16 is the largest square grid) or BV > 65535.  LP_ERR_ARGUMENT: a null images / out /
 * mask_out, H < patch or W < patch, count outside [0, N].  Any H, W: 16-byte accesses when W % 4 == 0, patch % 4 == 0 and both pointers
 * are 16-byte aligned, 4-byte ones otherwise.
 * ------------------------------------------------------------------------------------------------------ */
int lp_patch_mask_f32(const float* images, int BV, int C, int H, int W, int patch, int count, unsigned long long key, const float* mask_in,
                      float* out, float* mask_out, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Multi-view labeled batches with the 3-D augmentation (csrc/mv3d.hip; reference data/datasets.py:853-1104,
 * MultiviewHeatmapDataset.apply_3d_transforms and what it calls).  All fp32 unless said otherwise.
 *
 * lp_mv3d_plan: ONE launch for the batch, one workgroup per sample, no workspace, no atomics, every median a rank selection and every
 * sum in a fixed order: the same input gives the same bits.
 *   kp (B, V, K, 2) labels in stored-image px, NaN = unlabeled; src_hw (B, V, 2) stored image (height, width); bbox (B, 4 V) [x, y, h, w]
 *   per view; intrinsics / extrinsics / dist12 as for lp_cam_*; draws (B, 4) = [scale, r_x, r_y, r_z] drawn by the caller.
 *   1. frame px: u = x / ws * bw + bx, v = y / hs * bh + by.
 *   2. undistort + triangulate every pair (lp_cam_chain_fwd's arithmetic; a pair with a NaN point is NaN); X[k] = numpy's nanmedian over
 *      the pairs per coordinate (an even count: the mean of the two middle values; all NaN: NaN).
 *   3. status 2: every kp coordinate is NaN.  status 1: augment == 0, or fewer than 3 keypoints with a non-NaN X.  In both
 *      kp3d = X, kp2d = the labels in model px (x / ws * W, y / hs * H, NaN kept), affine = identity.
 *   4. otherwise med = nanmedian_k X; X' = (X - med) scale + med; extent = nanmax_k X' - nanmin_k X'; X' += shift_param extent r;
 *      q = X' projected into every view in frame px (lp_cam_project_fwd without a bbox; a NaN X' gives NaN).
 *   5. per view the least-squares similarity M_v = [[a, -b, t_x], [b, a, t_y]], stored px -> warped px, of o = kp onto
 *      n = ((q_x - bx) / bw ws, (q_y - by) / bh hs) over the keypoints finite in both: with o', n' centred on their means,
 *      a = sum o' . n' / sum |o'|^2, b = sum (o'_x n'_y - o'_y n'_x) / sum |o'|^2, t = mean n - R mean o; a zero denominator: identity.
 *      This is what cv2.estimateAffinePartial2D returns when every point is an inlier, up to its refinement tolerance (UNPINNED: cv2 is
 *      not a dependency).  Fewer than 3 matched keypoints in ANY view: status 3 and the outputs of status 1 for the whole sample - the
 *      reference raises RuntimeError("... should have been caught earlier") there.
 *   6. status 0: kp3d = X', kp2d = ((q_x - bx) / bw W, (q_y - by) / bh H) (not clipped), affine = M.
 *   kp3d (B, K, 3), kp2d (B, V, K, 2), affine (B, V, 2, 3), status (B) int32.  2 <= V <= LP_MV3D_MAX_VIEWS, K <= LP_MV3D_MAX_KEYPOINTS,
 *   B <= 65535 (LP_ERR_UNSUPPORTED otherwise); a null pointer or a non-positive dimension: LP_ERR_ARGUMENT.
 *
 * lp_mv3d_fill: src_u8 (B, Hs, Ws, 3) contiguous -> fill (B) = min over pixels and channels of (v / 255 - mean_c) / std_c (the reference
 * pads the warp with orig_img.min() of the normalised image).  One workgroup per sample.  std must be > 0.
 *
 * lp_mv3d_finish: normalise -> warp_affine(M, bilinear, align_corners=True, padding_mode="fill", same size) -> resize to (H, W)
 * (bilinear, half-pixel centres, no antialiasing, clamped taps: torch.nn.functional.interpolate's arithmetic) in ONE pass for ONE view:
 * output pixel (y, x) takes its 4 resize taps at integer warped pixels (X, Y); each tap is the bilinear sample of the normalised source
 * at M^-1 (X, Y) in pixel-index coordinates, a neighbour outside the image reading fill[b] (kornia's mask blend).  The warped image is
 * never written; M is inverted once per image (a singular or NaN M gives fill everywhere).  src_u8 (B, Hs, Ws, 3) is view v's images;
 * affine (B, V, 2, 3) is lp_mv3d_plan's output, row (b, v) is used; dst (B, V, 3, H, W): only [:, v] is written (16-byte stores when
 * W % 4 == 0 and dst is 16-byte aligned).  Views may differ in (Hs, Ws): one launch per view.  An identity M gives the plain resize of
 * the normalised image bit for bit (products and sums are not contracted).
 * ------------------------------------------------------------------------------------------------------ */
#define LP_MV3D_MAX_VIEWS 8
#define LP_MV3D_MAX_KEYPOINTS 128
int lp_mv3d_plan(const float* kp, const float* src_hw, const float* bbox, const float* intrinsics, const float* extrinsics,
                 const float* dist12, const float* draws, int augment, float shift_param, int H, int W, int B, int V, int K, float* kp3d,
                 float* kp2d, float* affine, int* status, lp_stream_t stream);
int lp_mv3d_fill(const void* src_u8, int B, int Hs, int Ws, const lp_frame_norm* norm, float* fill, lp_stream_t stream);
int lp_mv3d_finish(const void* src_u8, int B, int Hs, int Ws, const float* affine, const float* fill, const lp_frame_norm* norm, int V,
                   int v, int H, int W, float* dst, lp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Optimiser: torch.optim.Adam / AdamW semantics (models/base.py:458-479) over one flat fp32 range, also emitting
 * the bf16 copy the GEMMs read.  lr may be 0 (frozen backbone, callbacks.py:79-196): moments still move.
 * ------------------------------------------------------------------------------------------------------ */
int lp_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int decoupled, int step, float grad_scale, void* params_bf16, lp_stream_t stream);
int lp_cast_bf16(const float* src, size_t n, void* dst, lp_stream_t stream);
/* dst[c][b][a] = src[a][b][c] on bf16: weights [Co][R*S][Ci] -> data-gradient copy [Ci][R*S][Co] */
int lp_permute_cba(const void* src, int A, int B, int C, void* dst, lp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LP_HIP_H */
