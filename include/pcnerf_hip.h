/* pcnerf_hip.h -- C ABI of the MI355X (gfx950) PC-NeRF render + loss path.
 *
 * The reference (biter0088/pc-nerf) has no FFI: its hot path is eager PyTorch called from Python
 * (nof/render.py, nof/networks/models.py, nof/criteria/loss.py).  This library is what that Python
 * boundary binds to: the drop-in modules under pc-nerf_amd/nof/ keep the reference's names and signatures
 * and call these entry points through ctypes.  Every entry point below names the
 * reference code it replaces.
 *
 * Conventions
 *   - every pointer is a device pointer (hipMalloc'd / torch CUDA tensor) unless stated otherwise;
 *   - `stream` is a hipStream_t (NULL = legacy default stream); all work is enqueued asynchronously on it;
 *   - arrays are contiguous, fp32 unless stated; "rays" rows are `ray_stride` floats apart;
 *   - return value 0 = success; nonzero = failure, with a message from pcnerf_last_error()
 *     (argument errors are detected on the host before anything is launched).
 */
#ifndef PCNERF_HIP_H
#define PCNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCNERF_ABI_VERSION 1
#define PCNERF_FEATURES 256 /* NOF feature_size supported by the kernels (models.py:45 default) */
#define PCNERF_IN_CH 63     /* 3 + 3*2*L_pos with L_pos = 10 (train_kitti.py:25-28)            */

int pcnerf_abi_version(void);
const char* pcnerf_last_error(void);

/* ---------------------------------------------------------------- NOF network (models.py:44-359)
 * Parameters in reference state_dict order: Linear weights [256,63],[256,256]x3,[256,319],[256,256]x3
 * (layer1.{0,3,6,9}, layer2.{0,2,4,6}), BatchNorm1d gamma/beta/running_mean/running_var
 * (layer1.{1,4,7,10}, layer2.{1,3,5,7}), occ_out.0 weight [1,256] and bias [1]. */
typedef struct pcnerf_nof_params {
  const float* lin_w[8];
  const float* lin_b[8];
  const float* bn_w[8];
  const float* bn_b[8];
  float* bn_rm[8]; /* running_mean: read in eval mode, updated in place in train mode */
  float* bn_rv[8]; /* running_var:  idem */
  const float* out_w;
  const float* out_b;
} pcnerf_nof_params;

/* Eval-mode network image: BatchNorm (running stats) folded into each Linear, weights repacked into the
 * MFMA operand order of the fused query kernels -- the fp32 image followed by the split-fp16 image (per-layer
 * power-of-two scales, hi/mid fp16 parts).  Replaces the per-call nn.Module forward in eval mode. */
size_t pcnerf_nof_eval_packed_floats(void);
int pcnerf_nof_pack_eval(const pcnerf_nof_params* params, float* packed, void* stream);

/* Arithmetic of the fused eval-mode query (pcnerf_nof_query_eval / pcnerf_nof_forward_eval), process-wide;
 * returns the previous mode, or -1 for an invalid one.  0: fp32 MFMA (v_mfma_f32_32x32x2_f32).  1 (default): each
 * fp32 operand as two fp16 parts (22 significant bits; weights scaled per layer, activations per sample by powers
 * of two) and hi*hi + hi*mid + mid*hi on v_mfma_f32_32x32x16_f16 (exact products, fp32 accumulation), as
 * pcnerf_set_train_math mode 1. */
int pcnerf_set_eval_math(int mode);

/* Workgroup geometry of the split-fp16 fused queries (the eval query and the store-less train-mode query),
 * process-wide; returns the previous setting, or -2 for an invalid one.  -1 (default): each query's measured
 * default.  0..3: bit 0 = one 8-wave workgroup of 96 samples per CU (each wave 2 of a layer's 16 neuron blocks)
 * instead of two 4-wave workgroups of 48; bit 1 = a 4-slot weight ring instead of 2 slots.  Every geometry computes
 * the same bits; the setting exists for A/B timing and the bit-identity tests. */
int pcnerf_set_query_geometry(int geometry);

/* Form of the store-less train-mode query where it runs as the 8-wave workgroup with the 2-slot ring (query geometry
 * -1 or 1), process-wide; returns the previous setting, or -2 for an invalid one.  -1 (default): the measured
 * default (form 4; form 2 on a device that cannot give a workgroup 163,840 B of LDS, with a message in
 * pcnerf_last_error).  0: 6 sample blocks, 96 samples per pass over the weight image.  2: 7 sample blocks, 112 samples
 * per pass.  4: 8 sample blocks, 128 samples per pass, the activations and encoding operands as the CU's whole LDS.
 * (1 was a half-skewed schedule of form 0; it measured slower and is not built: refused, as are 3 and 5.)  Every form
 * computes the same bits; for A/B timing and the bit-identity tests. */
int pcnerf_set_train_query_form(int form);

/* Fused eval-mode query: for every flattened sample g = ray*n_samples + s computes
 *   p_out[g] = NOF(Embedding(o + d*z[g]))        (render.py:18-25 chunk loop, models.py:27-41, :183-203)
 * with o = rays[ray, 0:3], d = rays[ray, 3:6]. */
int pcnerf_nof_query_eval(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                          const float* packed, float* p_out, void* stream);

/* NOF.forward on an already embedded batch: p_out[i] = NOF(emb[i, 0:63]) (eval mode, packed image). */
int pcnerf_nof_forward_eval(const float* emb, int64_t n, const float* packed, float* p_out, void* stream);

/* Exact affine fold of the eval network (opt-in fast path): LeakyReLU(True) is the identity
 * (models.py:72,152,232) and eval BatchNorm is affine, so NOF(e) = sigmoid(a . e + c).  Writes fold[0..62] = a,
 * fold[63] = c (64 doubles), composed in float64 from the module's parameters (models.py:44-123, :183-203). */
int pcnerf_nof_fold_eval(const pcnerf_nof_params* params, double* fold, void* stream);

/* pcnerf_nof_query_eval through the fold: p_out[g] = sigmoid(fl32(a . Embedding(o + d*z[g]) + c)).  Replaces the
 * same eval chunk loop (render.py:18-25); rounding differs from the layer-by-layer network (~1e-7 rel logit). */
int pcnerf_nof_query_eval_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                               const double* fold, float* p_out, void* stream);

/* pcnerf_nof_forward_eval through the fold: p_out[i] = sigmoid(fl32(a . emb[i, 0:63] + c)). */
int pcnerf_nof_forward_eval_fold(const float* emb, int64_t n, const double* fold, float* p_out, void* stream);

/* Embedding(3, 10).forward (models.py:27-41): out[i, 0:63] = [x, sin(2^k x), cos(2^k x)]_k for x = pts[i, 0:3]. */
int pcnerf_embed(const float* pts, int64_t n, float* out, void* stream);

/* Train-mode query (BatchNorm batch statistics per chunk of `chunk` flattened ray-major samples, running
 * stats updated once per chunk with `momentum`; render.py:47-50 + nn.BatchNorm1d train semantics).
 * `workspace` must hold pcnerf_nof_train_workspace_bytes(chunk) bytes. */
size_t pcnerf_nof_train_workspace_bytes(int64_t chunk);
int pcnerf_nof_query_train(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                           int64_t chunk, const pcnerf_nof_params* params, float momentum, float eps,
                           void* workspace, size_t workspace_bytes, float* p_out, void* stream);

/* Arithmetic of the train-mode Linear layers (forward and the backward's forward recomputation), process-wide;
 * returns the previous mode, or -1 for an invalid one.  0: fp32 MFMA (v_mfma_f32_32x32x2_f32, an fp32 FMA chain).
 * 1 (default) / 2: each fp32 operand split into two fp16 parts (22 significant bits, power-of-two scaled) and the
 * products taken on the fp16 matrix pipe (v_mfma_f32_32x32x16_f16: exact products, fp32 accumulation):
 * hi*hi + hi*mid + mid*hi (1) or + mid*mid (2).  Measured against a float64 evaluation of the render:
 * as accurate as mode 0.  The reference's own GPU runs used TF32 matmuls (train_kitti.py:267). */
int pcnerf_set_train_math(int mode);

/* NOF.forward in train mode on an embedded batch of n rows (one BatchNorm chunk; running stats updated). */
int pcnerf_nof_forward_train(const float* emb, int64_t n, const pcnerf_nof_params* params, float momentum,
                             float eps, void* workspace, size_t workspace_bytes, float* p_out, void* stream);

/* ---------------------------------------------------------------- training backward (loss.backward())
 * Parameter gradients of the train-mode query, i.e. what autograd produces through render.py:47-50 and
 * models.py:183-203 (Linear -> BatchNorm1d(train) x 8, skip concat, occ_out, sigmoid) in the reference's
 * training step (train_kitti.py:155 `loss` returned to Lightning, which calls backward).  The chunks are
 * recomputed (same BatchNorm batches as the forward, running stats untouched).  Gradients are ADDED to the
 * non-NULL buffers of `grads` (torch .grad accumulation semantics); each has the shape of its parameter. */
typedef struct pcnerf_nof_grads {
  float* lin_w[8];
  float* lin_b[8];
  float* bn_w[8];
  float* bn_b[8];
  float* out_w;
  float* out_b;
} pcnerf_nof_grads;
size_t pcnerf_nof_backward_workspace_bytes(int64_t chunk);
/* grad_logit[g] = dL/d(occupancy logit) of flattened sample g (pcnerf_composite_backward's output). */
int pcnerf_nof_query_train_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                    int n_samples, int64_t chunk, const pcnerf_nof_params* params, float eps,
                                    const float* grad_logit, void* workspace, size_t workspace_bytes,
                                    const pcnerf_nof_grads* grads, void* stream);
/* Activation store (the training step without the backward's recomputation): pcnerf_nof_store_bytes(chunk) bytes
 * per chunk hold that chunk's raw layer outputs h_1..h_8 and BatchNorm statistics.  The _store forward writes
 * chunks 0..store_chunks-1 into `store` (results otherwise identical to pcnerf_nof_query_train); the _store
 * backward reads them instead of recomputing those chunks (the rest are recomputed).  The caller sizes
 * store_chunks to the HBM it can spare (nof._autograd: what is free after the backward workspace). */
size_t pcnerf_nof_store_bytes(int64_t chunk);
int pcnerf_nof_query_train_store(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                 int64_t chunk, const pcnerf_nof_params* params, float momentum, float eps,
                                 void* workspace, size_t workspace_bytes, float* p_out, void* store,
                                 int64_t store_chunks, void* stream);
int pcnerf_nof_query_train_backward_store(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                          int n_samples, int64_t chunk, const pcnerf_nof_params* params, float eps,
                                          const float* grad_logit, void* workspace, size_t workspace_bytes,
                                          const pcnerf_nof_grads* grads, const void* store, int64_t store_chunks,
                                          void* stream);
/* NOF.forward(emb) in train mode (one batch): grad_p = dL/dp for p = the forward's output. */
int pcnerf_nof_forward_train_backward(const float* emb, int64_t n, const pcnerf_nof_params* params, float eps,
                                      const float* p, const float* grad_p, void* workspace, size_t workspace_bytes,
                                      const pcnerf_nof_grads* grads, void* stream);

/* ---------------------------------------------------------------- opt-in train-mode affine fold
 * Exact affine fold of the TRAIN-mode network (SURVEY fact 1 with BatchNorm batch statistics; not the default --
 * the drop-in evaluates the module as written).  Every LeakyReLU(True) is the identity (models.py:72,152,232), so
 * within one BatchNorm chunk (render.py:47-50) every layer's batch mean and variance follow exactly from the
 * chunk's encoding mean and covariance, and NOF(e) = sigmoid(a_c . e + c_c) per chunk c (models.py:183-203).  The
 * forward computes those per-chunk moments, the float64 layer algebra, p_out and the running-stat updates (chunk by
 * chunk, as pcnerf_nof_query_train); `state` (pcnerf_nof_train_fold_bytes(total_samples, chunk) bytes) keeps what
 * the backward needs and must stay unchanged until it runs.  The backward ADDS the parameter gradients (the
 * Linear biases and the shifts of BatchNorms 0-6 are exactly zero there: the next BatchNorm removes the mean). */
size_t pcnerf_nof_train_fold_bytes(int64_t total_samples, int64_t chunk);
int pcnerf_nof_query_train_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                int64_t chunk, const pcnerf_nof_params* params, float momentum, float eps,
                                void* state, size_t state_bytes, float* p_out, void* stream);
int pcnerf_nof_forward_train_fold(const float* emb, int64_t n, const pcnerf_nof_params* params, float momentum,
                                  float eps, void* state, size_t state_bytes, float* p_out, void* stream);
int pcnerf_nof_query_train_fold_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                         int n_samples, int64_t chunk, const pcnerf_nof_params* params, float eps,
                                         const float* grad_logit, void* state, size_t state_bytes,
                                         const pcnerf_nof_grads* grads, void* stream);
/* ---------------------------------------------------------------- train-mode query without activations
 * The render+loss forward's train-mode query (render.py:38-50 chunk loop over models.py:183-203 with BatchNorm batch
 * statistics per chunk; replaces the layer-by-layer pcnerf_nof_query_train where no backward needs the layer
 * outputs).  The network is evaluated AS WRITTEN, per sample, in one fused kernel (the 9 Linear layers on split-fp16
 * products, BatchNorm applied in each layer's epilogue); only the chunk statistics it needs come from the chunk's
 * encoding moments through the float64 layer algebra above -- exact because every LeakyReLU(True) is the identity
 * (negative_slope = 1, models.py:72,92).  Running stats are updated chunk by chunk as nn.BatchNorm1d does.  `state`:
 * pcnerf_nof_train_fused_bytes(total_samples, chunk) bytes of scratch (the fold's forward pieces only: no
 * backward state). */
size_t pcnerf_nof_train_fused_bytes(int64_t total_samples, int64_t chunk);
int pcnerf_nof_query_train_fused(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                 int64_t chunk, const pcnerf_nof_params* params, float momentum, float eps,
                                 void* state, size_t state_bytes, float* p_out, void* stream);
/* The same query writing chunks 0..store_chunks-1 into an activation store (pcnerf_nof_store_bytes(chunk) bytes per
 * chunk, the layout pcnerf_nof_query_train_store writes: raw layer outputs W_L x and BatchNorm sums) for
 * pcnerf_nof_query_train_backward_fused (or _store).  Here `state` is pcnerf_nof_train_fold_bytes(total_samples,
 * chunk) bytes and must stay untouched until that backward: it holds the chunks' encoding moments and layer maps. */
int pcnerf_nof_query_train_fused_store(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                       int n_samples, int64_t chunk, const pcnerf_nof_params* params, float momentum,
                                       float eps, void* state, size_t state_bytes, float* p_out, void* store,
                                       int64_t store_chunks, void* stream);
/* The training backward after pcnerf_nof_query_train_fused_store (the autograd of render.py:47-50 / models.py:183-203
 * in train_kitti.py:155's loss.backward(), as pcnerf_nof_query_train_backward): `state` is that forward's state.
 * Each stored chunk's layers run ONE pass each (data gradient, BatchNorm backward and weight gradient together,
 * g_{L-1} written over h_{L-1} in the store, which the call CONSUMES: a second backward on the same store would read
 * gradients as activations -- recompute instead); the BatchNorm-backward statistics per chunk
 * come from the state (the chunk's encoding and gradient moments, float64).  Chunks beyond store_chunks are
 * recomputed and take the two-pass backward.  Gradients are ADDED to `grads`. */
int pcnerf_nof_query_train_backward_fused(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                          int n_samples, int64_t chunk, const pcnerf_nof_params* params, float eps,
                                          const float* grad_logit, void* state, size_t state_bytes, void* workspace,
                                          size_t workspace_bytes, const pcnerf_nof_grads* grads, void* store,
                                          int64_t store_chunks, void* stream);
/* Data-parallel BatchNorm running statistics (replaces, for DP training, the per-process running-stat update of
 * nn.BatchNorm1d in train mode, models.py:183-203 under render.py:47-50's chunk loop; Lightning's DDP leaves them
 * per rank).  pcnerf_nof_train_bn_stats: each chunk's batch statistics of a fused / fold train query (or embedded
 * forward) read from its `state` right after the forward -- out [C][8][2][256] doubles, C = ceil(total / chunk):
 * the mean of h_L (bias included) and the biased variance.  pcnerf_bn_running_replay: running_mean / running_var of
 * `params` advanced over `n_chunks` such records in order with the forward's own update arithmetic; `ns` (device,
 * int64) holds each chunk's sample count.  nof/bn_sync.py gathers every rank's records and replays them in global
 * chunk order, so every rank ends with the same statistics. */
int pcnerf_nof_train_bn_stats(const void* state, size_t state_bytes, int64_t total_samples, int64_t chunk,
                              double* out, void* stream);
int pcnerf_bn_running_replay(const pcnerf_nof_params* params, float momentum, const double* stats, const int64_t* ns,
                             int64_t n_chunks, void* stream);
/* The training step's forward and backward without any activation store (the default training path since round 5;
 * replaces the autograd of render.py:47-50 / models.py:183-203 that train_kitti.py:155's loss.backward() runs).
 * pcnerf_nof_query_train_fused_state: the fused query above, keeping its `state` (pcnerf_nof_train_fold_bytes
 * (total_samples, chunk) bytes: the chunks' encoding moments and layer maps) for the backward; nothing else is
 * written.  pcnerf_nof_query_train_backward_remat: every chunk's layers in ONE pass each (data gradient, BatchNorm
 * backward, weight gradient), each layer's input h_{L-1} - mean rematerialised per tile from the chunk's encoding
 * through its exact layer map P'_{L-1} (identity activations, models.py:72: the premise of the statistics); `state`
 * is consumed (its Sigma products are overwritten), `workspace` is pcnerf_nof_backward_workspace_bytes(chunk) bytes;
 * train math 1 (f16x2_3) only.  Gradients are ADDED to `grads`. */
int pcnerf_nof_query_train_fused_state(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                       int n_samples, int64_t chunk, const pcnerf_nof_params* params, float momentum,
                                       float eps, void* state, size_t state_bytes, float* p_out, void* stream);
int pcnerf_nof_query_train_backward_remat(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                          int n_samples, int64_t chunk, const pcnerf_nof_params* params, float eps,
                                          const float* grad_logit, void* state, size_t state_bytes, void* workspace,
                                          size_t workspace_bytes, const pcnerf_nof_grads* grads, void* stream);
/* ---------------------------------------------------------------- fused queries on explicit sample positions
 * The queries above with a third sample source: pts (n, 3) float32, contiguous, the flattened ray-major sample
 * positions, each taken verbatim -- they need not lie on any ray (jittered or warped samples, a voxel grid).  The
 * encoding stays fused (no (n, 63) embedding is written) and the arithmetic is the ray-sourced queries': on
 * pts = fl(o + fl(d*z)) the results are bit-identical.  BatchNorm chunk c covers samples [c*chunk, min((c+1)*chunk, n)).
 * pcnerf_nof_points_eval: p_out[g] = NOF(Embedding(pts[g])) in eval mode -- inference_val's / inference's /
 *   inference_0525_2's chunk loop over the caller's samples_xy (render.py:18-25; models.py:27-41, :183-203).  Eval
 *   math 1 only (under eval math 0: pcnerf_embed + pcnerf_nof_forward_eval).
 * pcnerf_nof_points_train_fused: inference_train's train-mode chunk loop (render.py:44-51; models.py:27-41, :183-203
 *   with BatchNorm batch statistics per chunk, running stats updated chunk by chunk), forward only; `state` is
 *   pcnerf_nof_train_fused_bytes(n, chunk) bytes of scratch.
 * pcnerf_nof_points_train_fused_state: the same, keeping the pcnerf_nof_train_fold_bytes(n, chunk) `state` for the
 *   backward.  pcnerf_nof_train_bn_stats reads either state as it reads a ray query's.
 * pcnerf_nof_points_train_backward_remat: the autograd of that loop to the parameters, as
 *   pcnerf_nof_query_train_backward_remat: `state` is consumed, `workspace` is
 *   pcnerf_nof_backward_workspace_bytes(chunk) bytes, train math 1 (f16x2_3) only, gradients are ADDED to `grads`.
 *   No gradient is taken with respect to pts. */
int pcnerf_nof_points_eval(const float* pts, int64_t n, const float* packed, float* p_out, void* stream);
int pcnerf_nof_points_train_fused(const float* pts, int64_t n, int64_t chunk, const pcnerf_nof_params* params,
                                  float momentum, float eps, void* state, size_t state_bytes, float* p_out,
                                  void* stream);
int pcnerf_nof_points_train_fused_state(const float* pts, int64_t n, int64_t chunk, const pcnerf_nof_params* params,
                                        float momentum, float eps, void* state, size_t state_bytes, float* p_out,
                                        void* stream);
int pcnerf_nof_points_train_backward_remat(const float* pts, int64_t n, int64_t chunk,
                                           const pcnerf_nof_params* params, float eps, const float* grad_logit,
                                           void* state, size_t state_bytes, void* workspace, size_t workspace_bytes,
                                           const pcnerf_nof_grads* grads, void* stream);
/* NOF.forward(emb) in train mode on an embedded batch of n rows (one chunk), the same way. */
int pcnerf_nof_forward_train_fused(const float* emb, int64_t n, const pcnerf_nof_params* params, float momentum,
                                   float eps, void* state, size_t state_bytes, float* p_out, void* stream);
/* NOF.forward(emb) through the fold (one chunk of n rows); grad_p = dL/dp of its output p. */
int pcnerf_nof_forward_train_fold_backward(const float* emb, int64_t n, const pcnerf_nof_params* params, float eps,
                                           const float* p, const float* grad_p, void* state, size_t state_bytes,
                                           const pcnerf_nof_grads* grads, void* stream);

/* ---------------------------------------------------------------- sampling (render.py:429-454, :497-511)
 * z[ray, :] = linspace sampling of [rays[near_col], rays[far_col]] with n_samples points; if
 * n_parent < n_samples the segmented scheme is used: n_parent points over [near, far] and
 * n_samples - n_parent over [rays[child_near_col], rays[child_far_col]], merged by sort.  disparity != 0:
 * linear in inverse depth, z = 1/(1/near*(1-s) + 1/far*s) (render.py:565-567, use_disp). */
int pcnerf_sample_coarse(const float* rays, int64_t n_rays, int ray_stride, int near_col, int far_col,
                         int child_near_col, int child_far_col, int n_samples, int n_parent, int disparity, float* z,
                         void* stream);
/* Stratified perturbation z' = lower + (upper - lower) * (perturb * rand) (render.py:449-454). */
int pcnerf_perturb(const float* z, int64_t n_rays, int n_samples, float perturb, const float* rand, float* z_out,
                   void* stream);

/* The compositing kernels' ray group, process-wide; returns the previous setting, or -1 for an invalid one.
 * 0 (default): a whole 256-thread workgroup per ray when the batch has fewer than 2,048 rays of >= 512 samples (the
 * reference shell's 256 rays x 2,304 fine samples: all CUs busy, 9 samples per thread), one wave per ray otherwise;
 * 64 / 256 force either (A/B, tests).  Same results: every sum and scan runs in float64 and rounds once. */
int pcnerf_set_composite_group(int group);

/* ---------------------------------------------------------------- compositing + child losses
 * (render.py:51-61 and :75-159).  Per ray: w = p * cumprod(1-p) (+ noise_std*noise if noise != NULL),
 * w /= sum(w) + eps; depth = sum(w z).  If `rays` != NULL, also the child masks (inclusive, expansion
 * from 0 and from 2 m by 0.01 steps) and the per-ray loss terms:
 *   free_ray[r] = sum_s (w * !M0)^2,   sl1_ray[r] = SmoothL1(10 * depth_child, 10 * range). */
int pcnerf_composite(const float* p, const float* z, int64_t n_rays, int n_samples, const float* noise,
                     float noise_std, float eps, const float* rays, int ray_stride, int child_near_col,
                     int child_far_col, int range_col, float* weights, float* depth, float* free_ray,
                     float* sl1_ray, double* opac_row, float* depth2, void* stream);
/* (opac_row, nullable: per-ray sum of log(0.1+p)+log(1.1-p)+2.20727, render.py:224; depth2, nullable: z at the
 * rank of the last sample in the descending weight order, render.py:598-600.) */
/* depth2's order of equal weights (render.py:598 argsort(descending=True)): 0 (default) = stable, as torch sorts
 * these rows on the GPU where the reference runs render_rays (rows > 32 long: merge / radix sort); 1 = torch CPU's
 * std::sort (introsort) order, reproduced per tied row (at most 2048 samples per ray; checked before any launch). */
int pcnerf_set_depth2_order(int order);
/* mean = sum(x[0:n]) / denom, one float written to out (used for the opacity means). */
int pcnerf_mean_f64(const double* x, int64_t n, double denom, float* out, void* stream);

/* Backward of pcnerf_composite + the child losses (render.py:51-61, 75-159) to the occupancy logits:
 * grad_logit[r, s] = dL/d logit(p[r, s]) given grad_depth[r] = dL/d depth[r] (nullable = 0) and the device
 * scalars grad_free_loss = dL/d child_free_loss, grad_depth_loss = dL/d child_depth_loss (nullable = 0;
 * ignored when rays == NULL).  sub_nerf_test_num > 0 selects the divide branch (child ids in
 * rays[:, child_id_col]); `workspace` then needs pcnerf_composite_backward_workspace_bytes(sub_nerf_test_num).
 * The weights are not differentiated through sample_pdf (render.py:466 detaches the fine samples). */
size_t pcnerf_composite_backward_workspace_bytes(int sub_nerf_test_num);
int pcnerf_composite_backward(const float* p, const float* z, int64_t n_rays, int n_samples, const float* noise,
                              float noise_std, float eps, const float* rays, int ray_stride, int child_near_col,
                              int child_far_col, int range_col, int child_id_col, int sub_nerf_test_num,
                              const float* grad_depth, const float* grad_free_loss, const float* grad_depth_loss,
                              void* workspace, float* grad_logit, void* stream);

/* ---------------------------------------------------------------- eval-mode gradients to the sample geometry
 * The eval network is p = sigmoid(a . Embedding(x) + c) with (a, c) = `fold`, the 64 doubles of pcnerf_nof_fold_eval
 * (SURVEY fact 1), so d logit / d x = J(x)^T a with J = d Embedding / d x (models.py:27-41: the identity columns,
 * d sin(2^k x_m) = 2^k cos(2^k x_m), d cos(2^k x_m) = -2^k sin(2^k x_m)) -- exactly, whichever eval math computed p.
 * grad_logit is pcnerf_composite_backward's output.  The encoding is recomputed at the float32 position the forward
 * evaluated; the dots and the per-ray sums accumulate in float64 and round once; no atomics (bit-reproducible).
 * pcnerf_nof_points_eval_backward: grad_pts[g, 0:3] = grad_logit[g] * J(pts[g])^T a for pts (n, 3) taken verbatim --
 *   what autograd of inference_val's chunk loop (render.py:18-25) leaves in samples_xy.grad.  n == 0 succeeds without
 *   a launch (no pointer is then read: all may be NULL).
 * pcnerf_nof_query_eval_backward: with x_s = fl(o + fl(d * z[r, s])) (o = rays[r, 0:3], d = rays[r, 3:6], render.py:
 *   518-520 / :458) and g_s = grad_logit[r, s] * J(x_s)^T a, grad_rays6[r, 0:3] = sum_s g_s and grad_rays6[r, 3:6] =
 *   sum_s z[r, s] g_s -- what autograd of render_rays_val's eval pass (render.py:485-536) leaves in rays.grad[:, 0:6];
 *   z is a constant of the pass.  grad_rays6 is (n_rays, 6), contiguous.  ray_stride >= 6, n_samples >= 1;
 *   n_rays == 0 succeeds without a launch.  No argument is nullable otherwise. */
int pcnerf_nof_points_eval_backward(const float* pts, int64_t n, const double* fold, const float* grad_logit,
                                    float* grad_pts, void* stream);
int pcnerf_nof_query_eval_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                   const double* fold, const float* grad_logit, float* grad_rays6, void* stream);

/* ---------------------------------------------------------------- eval-mode gradients to the parameters
 * Frozen-BatchNorm training: what autograd leaves in the 34 parameters' .grad through render.py:38-163 / :13-36 and
 * models.py:103-123 with the module in eval mode (running statistics used, not updated).  The eval network is
 * logit = a(theta) . Embedding(x) + c(theta), so with g_s = dL/dlogit of sample s the parameter
 * gradients of a whole pass are those of ONE pseudo-sample: dL/dtheta = d/dtheta [a(theta) . m + c(theta) s0] with
 * m = sum_s g_s Embedding(x_s) (63 numbers) and s0 = sum_s g_s.  Two stages:
 *   moments  mom[0..62] = m, mom[63] = s0 in float64 (device, 64 doubles), the encoding recomputed with the forward's
 *            own arithmetic at the float32 position it evaluated, every term g_s e_s formed exactly in float64;
 *            per-workgroup partials in `workspace` summed in a fixed order, no atomics, launch geometry a function of
 *            the sample count alone (two runs give equal bits).  `workspace` takes
 *            pcnerf_nof_eval_pgrad_workspace_bytes(total samples) bytes, 8-byte aligned.
 *            _rays: x_s = fl(o + fl(d z[r, s])) (render.py:44-45 / :458); _points: pts (n, 3) verbatim;
 *            _embedded: emb (n, 63) given; p != NULL takes `grad` as dL/dp and forms dL/dlogit = grad p (1 - p).
 *   algebra  pcnerf_nof_eval_param_grads: the pseudo-sample's forward and backward through the 9 layers in float64;
 *            fl32(value) is ADDED to every non-NULL buffer of `grads` (a NULL one is skipped); the Linear-bias and
 *            BatchNorm-shift gradients are NOT zero here (no batch mean is removed).  bn_rm / bn_rv are read only.
 * The _param_backward entries run both stages (mom at the head of `workspace`); grad_logit is
 * pcnerf_composite_backward's output; pcnerf_nof_forward_eval_param_backward takes p = NOF.forward(emb)'s output and
 * grad_p = dL/dp.  Zero samples succeed without a launch (nothing is added, mom is not written); null or
 * short-workspace arguments are refused before any launch. */
size_t pcnerf_nof_eval_pgrad_workspace_bytes(int64_t total_samples);
int pcnerf_nof_eval_gmoments_rays(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                  const float* grad_logit, void* workspace, size_t workspace_bytes, double* mom,
                                  void* stream);
int pcnerf_nof_eval_gmoments_points(const float* pts, int64_t n, const float* grad_logit, void* workspace,
                                    size_t workspace_bytes, double* mom, void* stream);
int pcnerf_nof_eval_gmoments_embedded(const float* emb, int64_t n, const float* p, const float* grad, void* workspace,
                                      size_t workspace_bytes, double* mom, void* stream);
int pcnerf_nof_eval_param_grads(const pcnerf_nof_params* params, float eps, const double* mom,
                                const pcnerf_nof_grads* grads, void* stream);
int pcnerf_nof_query_eval_param_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                         int n_samples, const pcnerf_nof_params* params, float eps,
                                         const float* grad_logit, void* workspace, size_t workspace_bytes,
                                         const pcnerf_nof_grads* grads, void* stream);
int pcnerf_nof_points_eval_param_backward(const float* pts, int64_t n, const pcnerf_nof_params* params, float eps,
                                          const float* grad_logit, void* workspace, size_t workspace_bytes,
                                          const pcnerf_nof_grads* grads, void* stream);
int pcnerf_nof_forward_eval_param_backward(const float* emb, int64_t n, const pcnerf_nof_params* params, float eps,
                                           const float* p, const float* grad_p, void* workspace,
                                           size_t workspace_bytes, const pcnerf_nof_grads* grads, void* stream);

/* ---------------------------------------------------------------- importance resampling
 * z_fine[ray, :] = sort(cat(z, sample_pdf(mid(z), weights[:, 1:-1], n_importance, det = (u == NULL))))
 * (render.py:371-412, :463-467).  `u` [n_rays, n_importance] replaces torch.rand when not NULL. */
int pcnerf_resample(const float* z, const float* weights, int64_t n_rays, int n_samples, int n_importance,
                    const float* u, float* z_fine, void* stream);

/* Standalone sample_pdf(bins (R, n_bins), weights (R, n_bins-1), n_samples, det = (u == NULL)) -> out
 * (R, n_samples), unsorted (render.py:371-412). */
int pcnerf_sample_pdf(const float* bins, const float* weights, int64_t n_rays, int n_bins, int n_samples,
                      const float* u, float* out, void* stream);

/* ---------------------------------------------------------------- losses
 * Child free / depth losses from the per-ray terms (render.py:102-159).  sub_nerf_test_num == 0 selects
 * the plain branch (sum / n_rays, 0.1/n_rays * mean); > 0 the per-child "divide" branch over child ids
 * 1..sub_nerf_test_num read from child_id[r * id_stride].  out[0] = free loss, out[1] = depth loss.
 * `workspace` needs pcnerf_child_loss_workspace_bytes(sub_nerf_test_num) bytes. */
size_t pcnerf_child_loss_workspace_bytes(int sub_nerf_test_num);
int pcnerf_child_loss_reduce(const float* free_ray, const float* sl1_ray, int64_t n_rays, const float* child_id,
                             int id_stride, int sub_nerf_test_num, void* workspace, float* out, void* stream);

/* mean(loss(pred, target)) over elements where mask != 0 (mask may be NULL); kind 0 = MSE, 1 = L1,
 * 2 = SmoothL1(beta 1) (nof/criteria/loss.py:12-50 with nn.*Loss(reduction='mean')).  out: one float. */
int pcnerf_pointwise_loss(const float* pred, const float* target, const uint8_t* mask, int64_t n, int kind,
                          float* out, void* stream);
/* Its backward: grad_pred[i] = grad_out * d loss_i / d pred_i / count (0 where mask == 0); grad_out is a
 * device scalar. */
int pcnerf_pointwise_loss_backward(const float* pred, const float* target, const uint8_t* mask, int64_t n, int kind,
                                   const float* grad_out, float* grad_pred, void* stream);

/* Per-child range loss, the use_child_nerf_divide branch of train_kitti.py:125-142 (replaces its Python loop over
 * sub_nerf_test_num children): out = sum over child ids c in 1..N owning >= 1 ray of
 * post_scale * mean_{i in c} loss(pre_scale*pred_i, pre_scale*target_i) (the reference: pre 10, post 0.1*lambda).
 * Child ids are read from child_id[i * id_stride] (ray column 9).  The backward needs the forward's workspace
 * (per-child sums and counts, pcnerf_child_range_loss_workspace_bytes) unchanged; grad_out is a device scalar. */
size_t pcnerf_child_range_loss_workspace_bytes(int sub_nerf_test_num);
int pcnerf_child_range_loss(const float* pred, const float* target, int64_t n, const float* child_id, int id_stride,
                            int sub_nerf_test_num, int kind, float pre_scale, float post_scale, void* workspace,
                            float* out, void* stream);
int pcnerf_child_range_loss_backward(const float* pred, const float* target, int64_t n, const float* child_id,
                                     int id_stride, int sub_nerf_test_num, int kind, float pre_scale, float post_scale,
                                     const void* workspace, const float* grad_out, float* grad_pred, void* stream);

/* ---------------------------------------------------------------- two-step inference (render_rays_view_0525_2_2)
 * Per row (render.py:241-354 after the query): weights = composite(p) normalised with eps, the strict child
 * mask [rows[child_near_col], rows[child_far_col]] expanded from 0.01 by 0.01, the argmax of the weights
 * smoothed by `gauss` (2*radius+1 float64 taps = scipy gaussian_filter(sigma=5), reflect), at_peak = mask at
 * that argmax, child_sum = sum(w * mask), depth (method 2: child re-normalised, else sum(w z)), the per-row
 * opacity sum and points = o + depth * d (points may be NULL, weights may be NULL). */
int pcnerf_view_rows(const float* p, const float* z, int64_t n_rows, int n_samples, const float* rows, int row_stride,
                     int child_near_col, int child_far_col, int method, float eps, const double* gauss, int radius,
                     float* weights, float* depth, uint8_t* at_peak, float* child_sum, double* opac_row,
                     float* points, void* stream);
/* Ray-group walk (render.py:317-340) over other_interest_sub_nerf_number (int64, k-1 on a group's first row):
 * flags[r] = 1 for the effective row of every group; *opacity = mean opacity term over n_rows * n_samples. */
size_t pcnerf_view_walk_workspace_bytes(int64_t n_rows);
int pcnerf_view_walk(const int64_t* other, int64_t n_rows, const uint8_t* at_peak, const float* child_sum,
                     const double* opac_row, int n_samples, void* workspace, uint8_t* flags, float* opacity,
                     void* stream);

/* ---------------------------------------------------------------- ray tables (ray/AABB intersection)
 * float64 inputs: points (n,3) and origin (3) of one LiDAR frame in the block frame, child boxes as bounds6
 * (C,6) = [xmin,ymin,zmin,xmax,ymax,zmax] (already grown by 0.025), centers (C,3), parent6 (6) the parent block.
 * Train/val 15-column rows (nof/dataset/ipb2dmapping.py:736-768): rows needs n_points*15 floats; the row count
 * is written to *n_rows (device int64).  face_rule 0 = compute_far_bound0606 (KITTI, :119-172: min/max of every
 * face hit, rays that hit no face are dropped); 1 = compute_far_bound0406 (MaiCity, :82-114, :383-395: the first
 * two hits, every point in a child box yields a row; rays with fewer than two hits -- the reference's IndexError
 * -- are counted in *n_short, a device int, so the caller can raise). */
size_t pcnerf_rays_workspace_bytes(int64_t n_points);
int pcnerf_build_train_rays(const double* points, int64_t n_points, const double* origin, const double* centers,
                            const double* bounds6, int64_t n_children, const double* parent6, double surface_expand,
                            int face_rule, void* workspace, float* rows, int64_t* n_rows, int* n_short,
                            void* stream);
/* Two-step 13-column rows grouped per ray (eval_kitti_render.py:675-803; method 2 = every child hit, method 1 =
 * first hit with parent bounds): count pass (writes *n_rows, device int64) then emit pass with the same workspace;
 * rule 0 = KITTI (expansion step 0.05, column 10 = max(parent far, child far)), 1 = MaiCity (multi_frame_maicity,
 * eval_kitti_render.py:344-431: step 0.005, column 10 = parent far; pass its child boxes grown by 0.025);
 * ranges (M), other_interest_sub_nerf_number (M, int64), true_in (M, bool). */
int pcnerf_count_view_rows(const double* points, int64_t n_points, const double* origin, const double* bounds6,
                           int64_t n_children, const double* parent6, int method, int rule, void* workspace,
                           int64_t* n_rows, void* stream);
int pcnerf_emit_view_rows(const double* points, int64_t n_points, const double* origin, const double* bounds6,
                          int64_t n_children, const double* parent6, int method, int rule, void* workspace,
                          float* rows, float* ranges, int64_t* other, uint8_t* true_in, void* stream);
/* Uniform-grid child index (the hierarchical parent/child ray-AABB lookup): the child centres binned into cubic
 * cells, CSR layout, so the two row builders above test the children near a point or a ray instead of all of them.
 * The *_grid builders write bit for bit what the flat ones write.
 * pcnerf_build_child_grid: `grid` is a device buffer of pcnerf_child_grid_bytes(n_children) =
 *   256 + align256((2^22 + 1) * 4) + 2 * align256(n_children * 4) bytes (header, cell_start at the cell cap,
 *   cell_items and the sort's scratch).  Origin = the centres' minimum, floor((max - min) / cell) + 1 cells per
 *   axis; `cell` doubles until the grid has at most 2^22 cells (the header keeps the edge in use).  Items are
 *   ascending inside each cell, so the build is deterministic.  Non-finite centres and cell <= 0 are errors.  The
 *   call waits for `stream` once (the dimensions are decided on the host).  Bin the centres the query measures
 *   from: `centers` for train rows, the box midpoints (bounds6[c][a] + bounds6[c][3 + a]) / 2 for two-step rows.
 * pcnerf_build_train_rays_grid: the 10 nearest centres by expanding rings of cells around the point's cell, exact
 *   (ties by index as the flat scan); workspace of pcnerf_rays_grid_workspace_bytes(n_points).
 * pcnerf_count_view_rows_grid / pcnerf_emit_view_rows_grid: the candidates come from a walk of the ray's whole
 *   line through the grid (a superset of the 0.65 m filter, which is then applied unchanged); the count pass keeps
 *   per ray its expansion round and the child indices of its <= 64 hits, the emit pass redoes those face tests:
 *   pcnerf_rays_grid_workspace_bytes(n_points) = pcnerf_rays_workspace_bytes(n_points) +
 *   align256(n_points * (8 + 64 * 4)) bytes.
 * Each query reads the grid's header back first (it waits for `stream`) and refuses a grid built over another
 * number of children. */
size_t pcnerf_child_grid_bytes(int64_t n_children);
int pcnerf_build_child_grid(const double* centers, int64_t n_children, double cell, void* grid, size_t grid_bytes,
                            void* stream);
size_t pcnerf_rays_grid_workspace_bytes(int64_t n_points);
int pcnerf_build_train_rays_grid(const double* points, int64_t n_points, const double* origin,
                                 const double* centers, const double* bounds6, int64_t n_children,
                                 const double* parent6, double surface_expand, int face_rule, const void* grid,
                                 void* workspace, float* rows, int64_t* n_rows, int* n_short, void* stream);
int pcnerf_count_view_rows_grid(const double* points, int64_t n_points, const double* origin,
                                const double* bounds6, int64_t n_children, const double* parent6, int method,
                                int rule, const void* grid, void* workspace, int64_t* n_rows, void* stream);
int pcnerf_emit_view_rows_grid(const double* points, int64_t n_points, const double* origin, const double* bounds6,
                               int64_t n_children, const double* parent6, int method, int rule, const void* grid,
                               void* workspace, float* rows, float* ranges, int64_t* other, uint8_t* true_in,
                               void* stream);

/* ---------------------------------------------------------------- evaluation metrics
 * (nof/criteria/pointcloud_metrics.py:5-49, logs/.../render_result/print_metrics.py:31-133; exhaustive float64
 * nearest-neighbour search instead of open3d's KD-tree).  Clouds are (n, 3) float32 rows.
 * pcnerf_nn_distance: dist[i] = min_j |query[i] - ref[j]| (float64).
 * pcnerf_eval_pts: out = {cd, fscore, precision, recall} of eval_pts(pred, gt, threshold): precision over the
 *   gt points' nearest-pred distances, recall over the pred points' nearest-gt distances, cd = sum of the two
 *   means; `workspace` needs pcnerf_eval_pts_workspace_bytes(n_pred, n_gt) bytes.  out is device memory.
 * pcnerf_range_metrics: out = {sum |r_pred - r_gt|, count(|.| < threshold)} with ranges from `origin` (3 floats)
 *   over n aligned points (abs_error / acc_thres before the division by n). */
int pcnerf_nn_distance(const float* ref, int64_t n_ref, const float* query, int64_t n_query, double* dist,
                       void* stream);
size_t pcnerf_eval_pts_workspace_bytes(int64_t n_pred, int64_t n_gt);
int pcnerf_eval_pts(const float* pred, int64_t n_pred, const float* gt, int64_t n_gt, double threshold,
                    void* workspace, double* out, void* stream);
int pcnerf_range_metrics(const float* pred, const float* gt, const float* origin, int64_t n, double threshold,
                         double* out, void* stream);

/* ---------------------------------------------------------------- kernel timing (bench / profiling)
 * pcnerf_prof_enable(1) makes every subsequent launch record a HIP event pair on its stream; tags:
 * 0 eval query, 1 train hidden Linear, 2 train first Linear, 3 train skip Linear, 4 train occ_out,
 * 5 BN fold, 6 composite, 7 resample, 8 sampling, 9 composite backward, 10 weight-gradient GEMM,
 * 11 data-gradient GEMM, 12 other backward kernels, 13 eval/train fold per-sample query, 14 split-math weight
 * gradients, 15 fused first layers, 16 train-fold moments, 17 train-fold layer algebra.  pcnerf_prof_read synchronises the tag's events and returns
 * the summed duration, launch count and algorithmic FLOPs / bytes of those launches. */
int pcnerf_prof_enable(int on);
int pcnerf_prof_read(int tag, double* total_ms, int64_t* launches, double* flops, double* bytes);

/* What the fp16 matrix pipe sustains on this board: the headline query's instruction (v_mfma_f32_16x16x32_f16, B
 * operands from LDS, one wave per SIMD, 24 accumulators per wave) in a bare loop on random operands, launched back
 * to back for `seconds` (settle for the first half, timed with HIP events over the second).  *tflops = dense fp16
 * TFLOP/s, *clock_mhz = median shader clock of the timed launches.  No reference counterpart (measurement only). */
int pcnerf_mfma_ceiling(double seconds, double* tflops, double* clock_mhz, void* stream);

/* ---------------------------------------------------------------- scan-to-field registration
 * Replaces: render.py:13-36 (inference_val: embed, eval network, compositing) plus torch autograd of its depth to
 * the ray origins and directions, and the normal equations a Gauss-Newton pose solver builds from them (no
 * reference counterpart beyond autograd).  Argument errors of these entries return -1.
 *
 * pcnerf_render_depth_jac_fold: one render pass of a folded eval network (fold = pcnerf_nof_fold_eval's 64
 *   doubles) in one launch, whatever pcnerf_set_eval_math selects: p = sigmoid(fl32(a . Embedding(o + d z) + c))
 *   with pcnerf_nof_query_eval_fold's arithmetic (its bits), compositing (render.py:51-61, no noise) in float64
 *   from that p, each output rounded once:
 *   depth (n_rays), sumw (n_rays) = sum_s T_s p_s (unnormalised: the hit probability),
 *   weights_or_null (n_rays, n_samples) = w / (sumw + eps), jac6_or_null (n_rays, 6) = d depth / d rays[:, 0:6]
 *   with z constant: columns 0:3 sum_s g_s grad logit(x_s), 3:6 sum_s z_s g_s grad logit(x_s), g_s = d depth /
 *   d logit_s (pcnerf_composite_backward's recurrence with dL/ddepth = 1).  1 <= n_samples <= 1024.
 * pcnerf_gn_normal_eq: out30 (30 device doubles) = the upper triangle of H = sum w Jp^T Jp (21, row-major),
 *   b = sum w Jp^T r (6), cost = sum rho(r), n_valid, one pad word, over the valid rays (sumw >= min_sumw, depth
 *   finite, target finite and > 0).  r = depth - target; w = 1 for |r| <= huber_delta, else huber_delta / |r|
 *   (huber_delta <= 0: plain least squares); Jp = [J_o, o x J_o + d x J_d] is the Jacobian of the left pose
 *   perturbation T' = exp(xi) T, xi = (rho, phi), on the world-frame ray row (delta o = rho + phi x o,
 *   delta d = phi x d).  `workspace` needs pcnerf_gn_workspace_bytes(n_rays) bytes.  float64 sums in a fixed
 *   order, no atomics.  n_rays == 0 zeroes out30. */
int pcnerf_render_depth_jac_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z, int n_samples,
                                 const double* fold, float eps, float* depth, float* sumw, float* weights_or_null,
                                 float* jac6_or_null, void* stream);
size_t pcnerf_gn_workspace_bytes(int64_t n_rays);
int pcnerf_gn_normal_eq(const float* rays, int64_t n_rays, int ray_stride, const float* jac6, const float* depth,
                        const float* sumw, const float* target, double huber_delta, double min_sumw,
                        void* workspace, double* out30, void* stream);

/* ---------------------------------------------------------------- pose-hypothesis scoring
 * Replaces: per pose the rays of a scan (nof.registration.scan_rays), render.py:485-536 (render_rays_val at
 * perturb = 0, noise_std = 0: coarse depths, coarse pass, sample_pdf with det = True, sort, fine pass) on two
 * folded eval networks, and the cost sum of pcnerf_gn_normal_eq -- for n_poses poses in one launch plus a small
 * reduction, with nothing per sample through memory (no reference counterpart for the batch: the observation model
 * of Monte-Carlo localisation).  Argument errors return -1.
 *
 * pcnerf_score_poses_fold: points_sensor (n_beams, 3) float32, sensor frame; poses12 (n_poses, 12) float64 rows
 *   [R row-major (9), t (3)], sensor -> world; parent_box6 = [lo (3), hi (3)] float64; fold_coarse / fold_fine =
 *   pcnerf_nof_fold_eval's 64 doubles.  Per (pose, beam), in float64 and then cast once to float32: rng = |p|,
 *   d = R (p / rng) renormalised, o = t, far = the exit from the box by the slab test (never below near).  The render
 *   is pcnerf_sample_coarse, pcnerf_render_depth_jac_fold (weights), pcnerf_resample (u = NULL),
 *   pcnerf_render_depth_jac_fold (depth, sumw) with their arithmetic.  r = depth - rng; a beam is usable when rng is
 *   finite and > 0 and valid when usable, sumw >= min_sumw and depth finite; rho(r) = r^2 / 2, or
 *   huber_delta (|r| - huber_delta / 2) for |r| > huber_delta > 0.
 *   scores4 (n_poses, 4) float64 = [sum_valid rho(r), n_valid, sum_valid |r|, sum_usable sumw];
 *   depth_or_null, sumw_or_null (n_poses, n_beams) float32, which do not change a bit of scores4.
 *   3 <= n_samples, 1 <= n_importance, n_samples + n_importance <= 1024.  `workspace` needs
 *   pcnerf_score_poses_workspace_bytes(n_poses, n_beams) bytes (32 per four beams of a pose).  float64 sums in an
 *   order fixed by (n_poses, n_beams), no atomics: a pose scores the same bits alone or in a batch.
 *   n_poses == 0 or n_beams == 0 zeroes scores4 and launches nothing else. */
size_t pcnerf_score_poses_workspace_bytes(int64_t n_poses, int64_t n_beams);
int pcnerf_score_poses_fold(const float* points_sensor, int64_t n_beams, const double* poses12, int64_t n_poses,
                            const double* parent_box6, float near, int n_samples, int n_importance,
                            const double* fold_coarse, const double* fold_fine, float eps, double huber_delta,
                            double min_sumw, void* workspace, size_t workspace_bytes, double* scores4,
                            float* depth_or_null, float* sumw_or_null, void* stream);

/* ---------------------------------------------------------------- batched pose refinement
 * Replaces: the loop of nof.registration.register_scan_fold (per evaluation scan_rays, render.py:485-536 at
 * perturb = 0, noise_std = 0 on two folded eval networks with torch autograd of the fine depth to the ray,
 * pcnerf_gn_normal_eq, a 30-double read-back and a host-side numpy solve and se3_exp) -- for n_poses poses at once,
 * every step on the device and stream order the only synchronisation between evaluations (no reference counterpart
 * for the batch: the refinement stage of Monte-Carlo localisation, multi-start registration).  Argument errors
 * return -1 before anything is launched.
 *
 * The state of a pose is PCNERF_LM_STATE_DOUBLES = 64 doubles:
 *   [ 0..11] T_acc    the last accepted pose, [R row-major (9), t (3)], sensor -> world
 *   [12..23] T_trial  the pose the next evaluation renders
 *   [24..53] the accepted evaluation's normal30 row (pcnerf_gn_normal_eq's out30 layout: 21 of H, 6 of b, cost,
 *            n_valid, pad)
 *   [54] lambda   [55] status   [56] evaluations made   [57] accepted evaluations   [58..63] the last xi
 * status: 0 running, 1 converged (|xi| < xi_tol; T_trial includes that last step), 2 fewer than 6 valid beams (the
 * pose is not determined), 3 a zero pivot or a non-finite xi in the solve (T_trial = T_acc).  A pose with
 * status != 0 costs nothing further: its workgroups return at once and its state keeps every word.
 *
 * pcnerf_pose_normal_eq_fold: one evaluation of all running poses, pcnerf_score_poses_fold's operands and render
 *   (the same bits of depth and sumw), the fine pass with pcnerf_render_depth_jac_fold's Jacobian path, then
 *   pcnerf_gn_normal_eq's terms per beam on those float32 values and the float32 ray row.  The poses are the
 *   states' T_trial, or poses12_or_null (n_poses, 12) when state_or_null is NULL.  normal30 (n_poses, 30) float64;
 *   the row of a pose with status != 0 is zeroed.  depth_or_null, sumw_or_null (n_poses, n_beams) and jac6_or_null
 *   (n_poses, n_beams, 6) float32 do not change a bit of normal30 (rows of stopped poses are not written).
 *   3 <= n_samples, 1 <= n_importance, n_samples + n_importance <= 1024.  `workspace` needs
 *   pcnerf_pose_normal_eq_workspace_bytes(n_poses, n_beams) bytes (256 per four beams of a pose).  float64 sums in
 *   an order fixed by (n_poses, n_beams), no atomics.  n_poses == 0 launches nothing; n_beams == 0 zeroes normal30.
 * pcnerf_lm_init: state (n_poses, 64) <- T_acc = T_trial = poses12, lambda = damping, everything else 0.
 * pcnerf_lm_update: register_scan_fold's step for every running pose from its normal30 row, in float64: one more
 *   evaluation; n_valid < 6 -> status 2 and nothing else moves; else the evaluation is accepted when none was
 *   accepted yet or cost <= the accepted cost (lambda / 10 except on the first; a NaN cost is a rejection once
 *   something is accepted), otherwise rejected (lambda x 10); (H + lambda diag H) xi = -b of the accepted evaluation
 *   by elimination with partial pivoting; T_trial = se3_exp(xi) T_acc (nof.registration.se3_exp's branches and
 *   series); |xi| < xi_tol -> status 1.  eval_costs_or_null (n_poses, iters) float64 and accepted_or_null (n_poses,
 *   iters) uint8 receive the cost and the decision at column iter_index (0 <= iter_index < iters when given).
 * pcnerf_refine_poses_fold: pcnerf_lm_init, then iters x (pcnerf_pose_normal_eq_fold on the states, pcnerf_lm_update),
 *   enqueued on `stream` with no synchronisation.  Writes poses12_out (n_poses, 12) = T_trial, or T_acc for status
 *   2 / 3; the state rows; normal30 (the last evaluation's rows, also scratch); eval_costs (NaN where not
 *   evaluated) and accepted.
 * pcnerf_se3_apply: poses12_out[p] = se3_exp(xi6[p]) poses12[p], xi = (rho, phi), float64 (the motion-model update
 *   of a particle set). */
#define PCNERF_LM_STATE_DOUBLES 64
size_t pcnerf_pose_normal_eq_workspace_bytes(int64_t n_poses, int64_t n_beams);
int pcnerf_pose_normal_eq_fold(const float* points_sensor, int64_t n_beams, const double* poses12_or_null,
                               int64_t n_poses, const double* state_or_null, const double* parent_box6, float near,
                               int n_samples, int n_importance, const double* fold_coarse, const double* fold_fine,
                               float eps, double huber_delta, double min_sumw, void* workspace,
                               size_t workspace_bytes, double* normal30, float* depth_or_null, float* sumw_or_null,
                               float* jac6_or_null, void* stream);
int pcnerf_lm_init(const double* poses12, int64_t n_poses, double damping, double* state, void* stream);
int pcnerf_lm_update(const double* normal30, int64_t n_poses, double xi_tol, double* state,
                     double* eval_costs_or_null, uint8_t* accepted_or_null, int iter_index, int iters, void* stream);
int pcnerf_refine_poses_fold(const float* points_sensor, int64_t n_beams, const double* poses12, int64_t n_poses,
                             const double* parent_box6, float near, int n_samples, int n_importance,
                             const double* fold_coarse, const double* fold_fine, float eps, double huber_delta,
                             double min_sumw, double damping, double xi_tol, int iters, void* workspace,
                             size_t workspace_bytes, double* normal30, double* state, double* poses12_out,
                             double* eval_costs, uint8_t* accepted, void* stream);
int pcnerf_se3_apply(const double* xi6, const double* poses12, int64_t n_poses, double* poses12_out, void* stream);

/* ---------------------------------------------------------------- localisation against a map of blocks
 * The scoring and the refinement above with every pose rendered against its own parent block, in one launch for
 * the whole set (no reference counterpart: a PC-NeRF map is several blocks, each with its own pair of networks and
 * its own AABB).  A map is n_blocks >= 1 blocks: folds_coarse / folds_fine (n_blocks, 64) float64, row b =
 * pcnerf_nof_fold_eval's output of block b; boxes6 (n_blocks, 6) float64 rows [lo (3), hi (3)], which may overlap.
 * block_of_pose (n_poses) int32: the block of each pose; -1, and any index outside 0 .. n_blocks - 1, renders
 * nothing and is never used as an index.  For a pose with block b every output equals, bit for bit, what the
 * single-block entry gives for that pose with block b's folds and box.  A beam is clipped at the exit from its
 * block's box; nothing is composited across blocks unless asked: pcnerf_score_poses_through.  Argument errors return
 * -1 before anything is launched.
 *
 * pcnerf_assign_blocks: block_of_pose[p] = the block whose box contains t_p (lo + margin <= t <= hi - margin on all
 *   three axes, float64) with the largest clearance min_m min(t_m - lo_m, hi_m - t_m), the lowest index on equal
 *   clearance; -1 when none contains it or a component of t_p is NaN.
 * pcnerf_score_poses_map: pcnerf_score_poses_fold's operands and outputs; the scores4 row of a pose without a block
 *   is zero, its depth NaN and its sumw 0.  `workspace` needs pcnerf_score_poses_workspace_bytes.
 * pcnerf_pose_normal_eq_map: pcnerf_pose_normal_eq_fold's operands and outputs; the normal30 row of a pose without a
 *   block (as of a stopped pose) is zero and its per-beam rows are not written.  `workspace` needs
 *   pcnerf_pose_normal_eq_workspace_bytes.
 * pcnerf_refine_poses_map: pcnerf_refine_poses_fold with pcnerf_pose_normal_eq_map as the evaluation; the block of a
 *   pose is fixed for the call.  A pose without a block stops with status 2 at the first update (zero valid beams)
 *   and poses12_out returns its input bits. */
int pcnerf_assign_blocks(const double* poses12, int64_t n_poses, const double* boxes6, int n_blocks, double margin,
                         int32_t* block_of_pose, void* stream);
int pcnerf_score_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12, int64_t n_poses,
                           const int32_t* block_of_pose, int n_blocks, const double* boxes6, float near,
                           int n_samples, int n_importance, const double* folds_coarse, const double* folds_fine,
                           float eps, double huber_delta, double min_sumw, void* workspace, size_t workspace_bytes,
                           double* scores4, float* depth_or_null, float* sumw_or_null, void* stream);
int pcnerf_pose_normal_eq_map(const float* points_sensor, int64_t n_beams, const double* poses12_or_null,
                              int64_t n_poses, const double* state_or_null, const int32_t* block_of_pose,
                              int n_blocks, const double* boxes6, float near, int n_samples, int n_importance,
                              const double* folds_coarse, const double* folds_fine, float eps, double huber_delta,
                              double min_sumw, void* workspace, size_t workspace_bytes, double* normal30,
                              float* depth_or_null, float* sumw_or_null, float* jac6_or_null, void* stream);
int pcnerf_refine_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12, int64_t n_poses,
                            const int32_t* block_of_pose, int n_blocks, const double* boxes6, float near,
                            int n_samples, int n_importance, const double* folds_coarse, const double* folds_fine,
                            float eps, double huber_delta, double min_sumw, double damping, double xi_tol, int iters,
                            void* workspace, size_t workspace_bytes, double* normal30, double* state,
                            double* poses12_out, double* eval_costs, uint8_t* accepted, void* stream);

/* ---------------------------------------------------------------- scoring with beams carried through the blocks
 * pcnerf_score_poses_through: pcnerf_score_poses_map with every beam carried on through the blocks it crosses.
 *   Segment 0 is pcnerf_score_poses_map's render in block b_0 = block_of_pose[p], from near to the box exit.  With
 *   te the float64 exit of the segment just rendered, block b' != b_k with the ray interval [tin, tout] in its box
 *   (tout the entry's own exit expression before the clamp to near, tin its mirror image) is a candidate when
 *   tin <= te + seam_tol, tout > te, neither is NaN and (float)tout > (float)max(te, tin); the next block is the
 *   candidate with the largest tout, the lowest index on ties.  Segment k >= 1 is the same two-pass render of the
 *   unchanged ray (o is still the sensor) with block b_k's folds from near_k = (float)max(te, tin) to the far that
 *   pcnerf_score_poses_fold forms for box b_k at near = near_k; each segment has its own n_samples + n_importance
 *   samples and its fine depth and sumw (dv_k, sv_k) are rounded once to float32.  The chain, float64, every operation
 *   rounded separately, from T = 1, W = 0, N = 0: W += T sv_k; N += T (dv_k (sv_k + eps)); T = max(T (1 - sv_k), 0).
 *   It ends after segment k when k + 1 == max_segments, T <= min_transmittance or no block is a candidate.  One
 *   rendered segment: depth = dv_0, sumw = sv_0, pcnerf_score_poses_map's bits.  Otherwise depth = (float)(N / (W +
 *   eps)) and sumw = (float)W: the compositing of the concatenated sample lists.  scores4 sums these two numbers
 *   exactly as pcnerf_score_poses_map sums its own.  Space inside a gap of at most seam_tol is free; where boxes
 *   overlap, the earlier block owns the beam up to its own exit.  n_segments_or_null / last_block_or_null
 *   (n_poses, n_beams) int32: the segments rendered and the block of the last one; a pose without a block gets 0 and
 *   -1 (and a zero scores4 row, NaN depth, zero sumw).  1 <= max_segments <= 16, seam_tol >= 0 (metres),
 *   0 <= min_transmittance < 1.  `workspace` needs pcnerf_score_poses_workspace_bytes.  The per-beam outputs change
 *   no bit of scores4.  Argument errors return -1 before anything is launched. */
int pcnerf_score_poses_through(const float* points_sensor, int64_t n_beams, const double* poses12, int64_t n_poses,
                               const int32_t* block_of_pose, int n_blocks, const double* boxes6, float near,
                               int n_samples, int n_importance, const double* folds_coarse,
                               const double* folds_fine, float eps, double huber_delta, double min_sumw,
                               int max_segments, double seam_tol, double min_transmittance, void* workspace,
                               size_t workspace_bytes, double* scores4, float* depth_or_null, float* sumw_or_null,
                               int32_t* n_segments_or_null, int32_t* last_block_or_null, void* stream);

/* ---------------------------------------------------------------- particle-filter update (Monte-Carlo localisation)
 * Weights, effective sample size and systematic resampling of a particle set on the device, in float64, with no
 * host synchronisation: every scalar that steers a later launch (n_usable, u0, ess) is read from device memory.  No
 * atomics; launch geometry and summation order depend on n_particles alone.  Argument errors return -1.
 *
 * pcnerf_mcl_weights: scores4 (n, 4) = pcnerf_score_poses_map's rows, n_usable_dev one float64 on the device (the
 *   scan's beams with a finite range > 0).  mean_p = (cost_p + miss_cost (n_usable - n_valid_p)) / n_usable,
 *   logw_p = logw_prev_p - beta mean_p, -inf where block_of_pose[p] < 0, mean_p is not finite or the result is NaN
 *   or +inf.  With m = max logw and Z = sum exp(logw - m): w_p = exp(logw_p - m) / Z, logw_p <- logw_p - m - log Z,
 *   ess[0] = Z^2 / sum exp(logw - m)^2 (= 1 / sum w^2), best[0] = the lowest index attaining m, degenerate[0] = 0.
 *   No finite logw: w = 1 / n, logw = 0, ess = n, best = 0, degenerate = 1.  1 <= n <= 4,194,304.
 *   Precondition: block_of_pose holds -1 .. n_blocks - 1 (what pcnerf_assign_blocks writes).  The entry does not know
 *   n_blocks: an id >= n_blocks, which the render entries treat as "no block" (a zero scores4 row), is NOT given
 *   -inf here but the finite weight of a pose that missed every beam; map such ids to -1 first.
 * pcnerf_systematic_resample: c = the inclusive prefix sums of w (negative, NaN and infinite weights count as 0) by
 *   a fixed-order hierarchical scan in which a zero weight gives c_i == c_{i-1} exactly; C = c_{n-1};
 *   u_j = (j + u0) / n_out * C with u0_dev[0] in [0, 1) (anything else counts as 0);
 *   ancestors[j] = the first i with c_i > u_j, clamped to the last i with w_i > 0.  With ess_dev_or_null given (the
 *   ESS switch; n_out must equal n) and ess[0] >= ess_threshold nothing is resampled: ancestors = 0 .. n - 1 and
 *   logw_out = logw; otherwise logw_out = 0.  poses12_out (n_out, 12), blocks_out (n_out) and logw_out (n_out), each
 *   optional with its input, are gathered by the ancestors.  1 <= n <= 4,194,304 (one thread walks the
 *   ceil(n / 1024) block totals as a serial chain). */
size_t pcnerf_mcl_weights_workspace_bytes(int64_t n_particles);
int pcnerf_mcl_weights(const double* logw_prev, const double* scores4, const int32_t* block_of_pose,
                       int64_t n_particles, const double* n_usable_dev, double miss_cost, double beta,
                       void* workspace, size_t workspace_bytes, double* w, double* logw, double* ess, int32_t* best,
                       int32_t* degenerate, void* stream);
size_t pcnerf_systematic_resample_workspace_bytes(int64_t n_particles);
int pcnerf_systematic_resample(const double* w, int64_t n_particles, const double* u0_dev, int64_t n_out,
                               const double* ess_dev_or_null, double ess_threshold, const double* poses12_or_null,
                               const int32_t* blocks_or_null, const double* logw_or_null, void* workspace,
                               size_t workspace_bytes, int32_t* ancestors, double* poses12_out_or_null,
                               int32_t* blocks_out_or_null, double* logw_out_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCNERF_HIP_H */
