/* vpn_hip.h — C ABI of libvpn_hip.so, the MI355X (gfx950) implementation of the
 * volumetric-primitive hot path (surface sampler, Chamfer nearest-neighbour
 * reduction, primitive soft raster), forward and analytic backward.
 *
 * Conventions:
 *  - every pointer is DEVICE memory owned by the caller (outputs and workspaces
 *    included); the library allocates no device memory and keeps no state that a
 *    RESULT depends on (contrast: the reference's module-global renderer,
 *    vertex_renderer.py:7,18).  What it does keep per process: the optional launch
 *    profiler's event list (vpn_profile_enable/read), the "dynamic LDS limit
 *    already raised" marks of a few kernels (vpn_chamfer_bwd's is kept per
 *    device) and the cached VPN_CHAMFER_MODE / VPN_CHAMFER_R
 *    environment overrides -- one process per GPU is the intended deployment,
 *    several host threads driving one library instance are not supported;
 *  - all tensors are contiguous fp32 unless stated, indices are int32;
 *  - `stream` is a hipStream_t passed as void*; kernels are only enqueued, no
 *    entry point synchronises with the host (the reference syncs through
 *    .item() at vertex_renderer.py:30-35 and cuboid.py:96);
 *  - return value: 0 on success, a positive hipError_t value if a launch failed,
 *    or a negative VPN_E_* code for rejected arguments.  Unlike the reference's
 *    emd extension (emd_cuda.cu:236-281, result ignored at emd_module.py:56) the
 *    host binding must raise on non-zero.
 *
 * Each entry point cites the reference interface it replaces (file:line relative
 * to the reference root).  The Python binding a maintainer adds is in
 * INTEGRATION.md (ctypes).
 */
#ifndef VPN_HIP_H
#define VPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 9 with vpn_hotpath_tile_rider_fits (the host-side answer to "would vpn_hotpath_chamfer_fwd take the rider?") and
 * with the visualisation stage (vpn_vis_primitives, vpn_vis_mesh, vpn_vis_mesh_workspace): entries were added, none
 * changed, and the binding resolves every symbol by name when it loads the library, so a library without them is refused
 * there.  9: the evaluation stage (vpn_eval_state_size, vpn_eval_accumulate).  8: the batch augmentation stage (vpn_cutmix_*, vpn_mixup_*).  7: the GCN refinement stage (vpn_gcn_*).  6: vpn_emd_fwd_ex, vpn_emd_recovered_samples, vpn_emd_last_group.
 * 5 (round 4): vpn_vpdiv_fwd, vpn_camera_matrix, vpn_trainstep_finalize, vpn_trainstep_bwd (the reference's whole training
 * step in one autograd node).  4 (round 3): raster records are 16 float4 per primitive (vpn_raster_records_size grew), tile_order is a buffer of
 * 48-byte tile entries (vpn_raster_order_size, K <= 64).  3: vpn_raster_total_fwd_fin, vpn_hotpath_chamfer_fwd, the mesh
 * entry points. */
#define VPN_ABI_VERSION 9

/* primitive kinds (reference: train.py:106-116 cuboids first, then spheres, cones are stubs) */
#define VPN_SPHERE 0
#define VPN_CUBOID 1

/* negative return codes */
#define VPN_E_BADARG  (-1)   /* null pointer / non-positive size              */
#define VPN_E_TOOBIG  (-2)   /* size above a documented limit                 */

/* packed primitive parameters: [B, K, 10] = (v0 v1 v2 | q0 q1 q2 q3 | t0 t1 t2)
 * — the reference passes K separate (B,3),(B,4),(B,3) tensors (train.py:117).  */
#define VPN_PARAM_STRIDE 10
/* largest K the raster / sampler stage in LDS */
#define VPN_MAX_PRIMS 1024
/* largest cloud vpn_cutmix_points takes: the 2 N candidate keys of a sample live in one workgroup's LDS */
#define VPN_CUTMIX_MAX_POINTS 8192
/* largest cloud and most clusters vpn_cluster_points / vpn_support_hulls take: a sample's cloud (16 bytes a point) lives in
 * one workgroup's LDS */
#define VPN_CLUSTER_MAX_POINTS 8192
#define VPN_CLUSTER_MAX_HULLS 32
/* most hulls, directions, samples and candidates vpn_hull_augment / vpn_union_surface take: the directions (16 bytes each),
 * the G * D support values and the nc survivor indices of a sample live in one workgroup's LDS (132 KiB at the limits) */
#define VPN_UNION_MAX_HULLS 64
#define VPN_UNION_MAX_DIRS 256
#define VPN_UNION_MAX_SAMPLES 65535
#define VPN_UNION_MAX_CAND 16384
/* largest K vpn_vis_primitives takes: the records of one (sample, view) live in one workgroup's LDS (116 bytes each) */
#define VPN_VIS_MAX_PRIMS 512
/* faces per chunk of a ragged mesh batch (vpn_ragged_sample; the host's chunk table is cut with the same constant): one
 * 256-lane workgroup scans a chunk, four consecutive faces a lane; most point sets per mesh */
#define VPN_RAGGED_CHUNK 1024
#define VPN_RAGGED_MAX_SETS 16

int vpn_abi_version(void);
/* static description of a code returned by any entry point below */
const char* vpn_error_string(int code);

/* Optional per-kernel timing for benchmarks: while enabled, every kernel the library launches is
 * bracketed by a pair of HIP events on its stream (do not enable under graph capture).
 * vpn_profile_enable(on) clears the records; vpn_profile_read synchronises and returns, per kernel
 * name (newline separated in `names`), the mean duration in ms and the number of launches. */
int vpn_profile_enable(int on);
int vpn_profile_read(char* names, int names_len, float* mean_ms, int* calls, int max_entries);

/* ------------------------------------------------------------------ sampler
 * Replaces Sampling.sphere_sampling / cuboid_sampling (modules/sampling/
 * sampling.py:11-37, sphere.py:22-43, cuboid.py:8-101), transform_points
 * (modules/transform/transform.py:6-9) and the per-primitive loop + torch.cat of
 * sample_predict_points (train.py:105-120) in one launch.
 *   params [B,K,10], kinds [K] int32 (device), points [B, K*n, 3] primitive-major.
 *   u: explicit uniform draws [B,K,n,3] (sphere: u0 = elev draw, u1 = azim draw,
 *      sphere.py:26-27; cuboid: the three draws of cuboid.py:66), or NULL to
 *      generate them in-kernel with Philox4x32-10 keyed by (seed, sample_base+b,
 *      k, point) so the result does not depend on how the batch is sharded.
 *   seed_dev: NULL, or a DEVICE uint64 read when the kernel runs and added to `seed`: a step counter the
 *      caller bumps on the stream, so that a captured HIP graph replayed N times draws N different point
 *      sets like the reference's per-step torch.rand (sphere.py:26-27) instead of freezing the seed at capture.
 */
int vpn_sample_fwd(const float* params, const int32_t* kinds, const float* u,
                   uint64_t seed, const uint64_t* seed_dev, uint64_t sample_base, int B, int K, int n,
                   float* points, void* stream);
/* grad_params [B,K,10] is WRITTEN (not accumulated).  (seed, *seed_dev) must be what the forward saw. */
int vpn_sample_bwd(const float* params, const int32_t* kinds, const float* u,
                   uint64_t seed, const uint64_t* seed_dev, uint64_t sample_base, int B, int K, int n,
                   const float* grad_points, float* grad_params, void* stream);
/* Backward of ChamferDistanceLoss(sample(params), gt_points) straight to grad_params [B,K,10], for the pair of
 * calls train.py:117-120 + :160-161 makes: equals vpn_chamfer_bwd (gradient of the predicted cloud only, GT gets
 * none) followed by vpn_sample_bwd, without the [B,K*n,3] point gradient in between and in a fixed summation
 * order.  points [B,K*n,3] = what vpn_sample_fwd produced from the same (params, kinds, u | seed, sample_base);
 * dist/idx from vpn_chamfer_fwd*(points, gt_points); grad_loss_b [B] as in vpn_chamfer_bwd.
 * M <= VPN_FUSED_BWD_MAX_GT (VPN_E_TOOBIG beyond: use the two separate calls): the kernel keeps per-wave match lists of the
 * GT points in LDS, 8 bytes a point in 60 KB. */
#define VPN_FUSED_BWD_MAX_GT 7680
int vpn_sample_chamfer_bwd(const float* params, const int32_t* kinds, const float* u,
                           uint64_t seed, const uint64_t* seed_dev, uint64_t sample_base, int B, int K, int n,
                           const float* points, const float* gt_points, int M,
                           const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2,
                           const float* grad_loss_b, float w1, float w2, float* grad_params, void* stream);

/* ---------------------------------------------------------------- transform
 * Replaces transform_points / rotate_points (modules/transform/transform.py:6-9,
 * rotate.py:7-25, translate.py:4-8): out = R(q) p + t.  t may be NULL (pure
 * rotation).  points/out [B,N,3], q [B,4], t [B,3].
 */
int vpn_transform_fwd(const float* points, const float* q, const float* t,
                      int B, int N, float* out, void* stream);
/* grad_points [B,N,3], grad_q [B,4], grad_t [B,3] are written; any may be NULL. */
int vpn_transform_bwd(const float* points, const float* q, const float* grad_out,
                      int B, int N, float* grad_points, float* grad_q, float* grad_t,
                      void* stream);

/* ------------------------------------------------------------------ Chamfer
 * Replaces the dense B*N*M expression of ChamferDistanceLoss.forward
 * (modules/loss/chamfer_distance.py:14-23).  p1 [B,N,3], p2 [B,M,3].
 *   dist1[b,i] = min_j ||p1_i - p2_j|| (NON-squared), idx1 = argmin_j with the
 *   reference's tie rule (lowest index among equal sqrt values), dist2/idx2 the
 *   other direction.  Bit-exact with the fp32 reference expression.
 */
int vpn_chamfer_fwd(const float* p1, const float* p2, int B, int N, int M,
                    float* dist1, int32_t* idx1, float* dist2, int32_t* idx2, void* stream);
/* One direction only (one kernel launch): for every query point the nearest target point.
 * queries [B,Nq,3], targets [B,Nt,3] -> dist [B,Nq], idx [B,Nq].  vpn_chamfer_fwd is two of these. */
int vpn_chamfer_nn(const float* queries, const float* targets, int B, int Nq, int Nt,
                   float* dist, int32_t* idx, void* stream);
/* Both directions with a caller-provided workspace of vpn_chamfer_workspace(B,N,M) bytes: each
 * scan strategy is selectable and every strategy returns the same bits as vpn_chamfer_fwd:
 *   mode 1  brute force (workspace unused, may be NULL);
 *   mode 2  box-pruned: clouds Morton-sorted per call, target chunks farther than the current best skipped;
 *   mode 3  matrix-pipe filter: bf16 MFMA (fp32 coordinates split exactly into three bf16 pieces) evaluates
 *           |b|^2 - 2a.b for 32x32 pairs, the candidates are re-evaluated with the exact separately-rounded
 *           d2 (a rigorous error band decides when a second block or a full exact rescan is needed);
 *   mode 4  the same filter with fp32-input MFMA;
 *   mode 5  mode 3 over Morton-sorted clouds with per-block boxes (target blocks that cannot hold a nearer point skipped);
 *   mode 6  the filter with ONE fp16 MFMA per 32x32 block: coordinates scaled by 2^11 and split into two fp16
 *           pieces (32-byte rows); queries or clouds with |p|^2 > 64 are outside its domain and are finished by
 *           the exact rescan (results unchanged, only slower);
 *   mode 7  mode 6 with the features of both clouds already in the workspace (written by vpn_hotpath_sample_fwd
 *           for p1 = its points and p2 = its gt_points, earlier on the same stream);
 *   mode 0  automatic (mode 6 for large clouds when a workspace is given, else mode 1). */
size_t vpn_chamfer_workspace(int B, int N, int M);
/* workspace_bytes: size of `workspace`; VPN_E_BADARG if a mode that uses it is given fewer than
 * vpn_chamfer_workspace(B,N,M) bytes or a pointer that is not 16-byte aligned (the filtered scans fetch row
 * tiles without bounds checks inside it). */
int vpn_chamfer_fwd_ws(const float* p1, const float* p2, int B, int N, int M,
                       float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                       void* workspace, size_t workspace_bytes, int mode, void* stream);
/* loss_b[b] = w1*mean_i dist1[b,i] + w2*mean_j dist2[b,j]   (chamfer_distance.py:25-28) */
int vpn_chamfer_loss(const float* dist1, const float* dist2, int B, int N, int M,
                     float w1, float w2, float* loss_b, void* stream);
/* Backward of loss_b w.r.t. the points given grad_loss_b [B].  grad_p1 [B,N,3] /
 * grad_p2 [B,M,3] are written; either may be NULL.  A coincident pair gives NaN
 * like the reference's autograd (0/0).  An index outside the other cloud (the
 * filtered scans return 0x7fffffff for a point with a NaN or infinite coordinate)
 * is not read through: that point's row is NaN and the pair adds to no other row. */
int vpn_chamfer_bwd(const float* p1, const float* p2,
                    const float* dist1, const int32_t* idx1,
                    const float* dist2, const int32_t* idx2,
                    const float* grad_loss_b, int B, int N, int M, float w1, float w2,
                    float* grad_p1, float* grad_p2, void* stream);

/* ------------------------------------------------------------------- raster
 * Replaces VertexRenderer.render (modules/render/vertex_renderer.py:14-26) and the
 * per-sample loop of SilhouetteLoss.forward (modules/loss/silhouette.py:16-20):
 * one launch renders the whole batch straight from the primitive parameters (the
 * reference meshes the primitives first, modules/meshing/sphere.py:8-27, and
 * rasterises the mesh with kaolin's DIBRenderer, which is not in its tree).
 *   cam [B,3] = (dist, elev_deg, azim_deg)   (vertex_renderer.py:18)
 *   alpha, depth [B,H,W]; aux [B,3,H,W] = (prod(1-a), zbar, sum w) saved for bwd;
 *   records: vpn_raster_records_size(B,K,H,W) bytes, 16-byte aligned, written by fwd (the
 *   per-primitive camera-space ray coefficients and culling conics, then the per-tile
 *   visibility masks) and read again by bwd — keep it alive with aux.
 */
size_t vpn_raster_records_size(int B, int K, int H, int W);
int vpn_raster_fwd(const float* params, const int32_t* kinds, const float* cam,
                   int B, int K, int H, int W, float sigma, float gamma, float z_far,
                   float* alpha, float* depth, float* aux, void* records, void* stream);
/* bytes of workspace vpn_raster_bwd needs (16-byte aligned, contents scratch) */
size_t vpn_raster_bwd_workspace(int B, int K, int H, int W);
/* grad_alpha / grad_depth [B,H,W] (either may be NULL = zero); grad_params
 * [B,K,10] is written.  Bitwise reproducible (no atomics). */
int vpn_raster_bwd(const float* params, const int32_t* kinds, const float* cam,
                   int B, int K, int H, int W, float sigma, float gamma, float z_far,
                   const float* aux, const void* records,
                   const float* grad_alpha, const float* grad_depth,
                   void* workspace, float* grad_params, void* stream);

/* ------------------------------------------------ raster with fused image losses
 * SilhouetteLoss.forward (modules/loss/silhouette.py:13-23: render, then L1Loss or MSELoss mean
 * against the GT silhouette) in one pass, optionally with an L1 depth loss: the losses are
 * evaluated where the pixel is produced, so alpha/depth and their gradients never travel through HBM.
 *   gt_sil, gt_depth [B,H,W] (either may be NULL -> that loss is 0); sil_mse: 0 = L1, 1 = MSE;
 *   losses [4] = (mean silhouette loss, mean |depth - gt_depth|, their sum, 0);
 *   loss_ws: vpn_raster_loss_workspace(B,H,W) bytes of scratch (16-byte aligned); aux/records as for vpn_raster_fwd.
 */
size_t vpn_raster_loss_workspace(int B, int H, int W);
int vpn_raster_loss_fwd(const float* params, const int32_t* kinds, const float* cam,
                        int B, int K, int H, int W, float sigma, float gamma, float z_far,
                        const float* gt_sil, const float* gt_depth, int sil_mse,
                        float* aux, void* records, void* loss_ws, float* losses, void* stream);
/* grad_losses [2] (device): upstream gradients of the two scalar losses; workspace as for
 * vpn_raster_bwd; grad_params [B,K,10] is written, or added to when accumulate != 0 (so the gradient of
 * the sampler + Chamfer branch and of the raster branch meet without an extra pass). */
int vpn_raster_loss_bwd(const float* params, const int32_t* kinds, const float* cam,
                        int B, int K, int H, int W, float sigma, float gamma, float z_far,
                        const float* aux, const void* records,
                        const float* gt_sil, const float* gt_depth, int sil_mse,
                        const float* grad_losses, void* workspace, float* grad_params, int accumulate,
                        void* stream);

/* ---- the training step's image losses, forward and backward in ONE pass (train.py:243-262, :176)
 *   total_img = w_sil * SilhouetteLoss(render(params), gt_sil) + w_dep * mean |depth - gt_depth|
 * vpn_raster_total_fwd renders, evaluates both losses and, in the same kernel, the gradient of total_img w.r.t. the
 * ray coefficients (for an upstream gradient of 1; the result is linear in it): per-tile loss sums go to loss_ws,
 * gradient partials to `workspace` (vpn_raster_bwd_workspace bytes); no aux tensor exists.
 * vpn_loss_finalize turns the per-tile sums (and, when dist1/dist2 [B,N]/[B,M] are given, the per-sample Chamfer
 * loss cd_b = cd_w1 mean_i dist1 + cd_w2 mean_j dist2, chamfer_distance.py:25-28) into
 *   losses[4] = (silhouette loss, depth loss, w_cd * mean_b cd_b + w_sil * [0] + w_dep * [1], mean_b cd_b)
 * in a fixed summation order; loss_b [B] (optional) receives cd_b.  H = W = 0: no image losses (Chamfer only; loss_ws
 * then needs 16 + 16 B bytes, zeroed once by the caller).
 * vpn_raster_total_bwd (when backward runs): grad_params (+)= (*grad_total) * d total_img / d params from the
 * partials; grad_total is a DEVICE scalar (NULL = 1). */
/* records_ready != 0: `records` were already written (and the counter at the head of loss_ws zeroed) by
 * vpn_hotpath_sample_fwd for the same (params, kinds, cam, H, W, sigma): the record launch is skipped. */
int vpn_raster_total_fwd(const float* params, const int32_t* kinds, const float* cam,
                         int B, int K, int H, int W, float sigma, float gamma, float z_far,
                         const float* gt_sil, const float* gt_depth, int sil_mse, float w_sil, float w_dep,
                         void* records, void* loss_ws, void* workspace, int records_ready, void* stream);
/* vpn_raster_total_fwd and vpn_loss_finalize in ONE launch (what SilhouetteLoss and the training step use): the tile
 * wave that completes a sample sums that sample's tile losses, the one that completes the batch writes losses[4] as
 * vpn_loss_finalize defines them (fixed summation order: bitwise reproducible).  chamfer_ws != NULL: the workspace a
 * preceding vpn_chamfer_fwd_ws call on this stream ran its fp16 filter in (vpn_hotpath_fused_features(B, K, n, M) == 1,
 * modes 0 / 6 / 7): the per-sample Chamfer term cd_b = cd_w1 mean_i dist1 + cd_w2 mean_j dist2 (chamfer_distance.py:25-28)
 * is taken from the per-workgroup sums that scan left there, N and M are its cloud sizes; NULL: image losses only
 * (cd = 0).  loss_b [B] (optional) receives cd_b.  seed_advance (optional): a device uint64 that is incremented once
 * when the batch is complete -- the step counter vpn_hotpath_sample_fwd was given as seed_dev, so the next step draws
 * fresh surface points without a kernel of its own; the seed this step used stays readable at (char*)loss_ws + 8.
 * Ordering the in-kernel finalisation rests on: a tile wave publishes its two loss sums with write-through (sc1) stores,
 * waits for their acknowledgement (vmcnt(0)) and only then adds to its sample's arrival counter with a relaxed
 * agent-scope add; the wave whose add completes the sample reads the sums back with sc1 loads.  That is the hand-off
 * form gfx950 executes correctly (MI355X_MICROARCH.md lists it as valid, "not an architectural guarantee"); it is NOT
 * the HIP memory model's release / acquire pairing, which a build with -DVPN_STRICT_ORDER uses instead (same results,
 * 6x the kernel time: an L2 write-back and an L1 invalidate per tile wave).  Gradients do not depend on it.
 * tile_order (optional, needs records_ready and K <= 64): the tile entries vpn_hotpath_chamfer_fwd wrote -- launch order
 * of the tile waves (heaviest tile first), tile masks and quadrant masks; the tile masks inside `records` are then taken
 * as written too. */
int vpn_raster_total_fwd_fin(const float* params, const int32_t* kinds, const float* cam,
                             int B, int K, int H, int W, float sigma, float gamma, float z_far,
                             const float* gt_sil, const float* gt_depth, int sil_mse, float w_sil, float w_dep,
                             void* records, void* loss_ws, void* workspace, int records_ready,
                             const void* chamfer_ws, size_t chamfer_ws_bytes, int N, int M, float cd_w1, float cd_w2,
                             float w_cd, float* losses, float* loss_b, uint64_t* seed_advance, const void* tile_order,
                             void* stream);
/* vpn_sample_fwd of the training step: the same launch also writes the raster records of the primitives it samples
 * (one workgroup per (sample, primitive) in both) and zeroes the arrival counter of loss_ws.
 * chamfer_ws != NULL (allowed when vpn_hotpath_fused_features(B, K, n, M) is 1): the launch also writes, into that
 * Chamfer workspace (vpn_chamfer_workspace(B, K*n, M) bytes), the matrix-pipe filter's features of the cloud it
 * samples and of gt_points [B,M,3]; the caller then runs vpn_chamfer_fwd_ws(points, gt_points, ..., mode 7) on the same
 * workspace and stream, which skips its feature kernel (the points would be written and immediately re-read).
 * chamfer_ws == NULL: gt_points / M / chamfer_ws_bytes are ignored.  With a Chamfer workspace the records are built
 * by workgroups of their own at the head of the launch (one lane per primitive), not by the sampler workgroups. */
int vpn_hotpath_sample_fwd(const float* params, const int32_t* kinds, const float* u,
                           uint64_t seed, const uint64_t* seed_dev, uint64_t sample_base, int B, int K, int n,
                           float* points, const float* cam, int H, int W, float sigma, void* records, void* loss_ws,
                           const float* gt_points, int M, void* chamfer_ws, size_t chamfer_ws_bytes,
                           void* stream);
int vpn_hotpath_fused_features(int B, int K, int n, int M);
/* The Chamfer scan of the training step (vpn_chamfer_fwd_ws with the fp16 filter: mode 0 where it resolves to it, 6 or 7)
 * with a RIDER in the same launch: behind the scan's workgroups, in the tail of the launch where slots idle, one
 * workgroup per image tests that image's 16x16 tiles and their 8x8 quadrants against its K primitives (the visibility
 * test of the tile kernels), writes the tile masks into `records` (as written by vpn_hotpath_sample_fwd earlier on this
 * stream) and tile_order (vpn_raster_order_size bytes, 16-byte aligned): one 48-byte entry per (image, launch rank) =
 * (tile, number of visible primitives, their mask, four quadrant masks), the tiles of every image sorted by visible
 * primitives, heaviest first -- what a tile wave of vpn_raster_total_fwd_fin needs to know, in one load (the second half
 * of the buffer is the rider's scratch: the same entries by tile).  tile_order == NULL: exactly vpn_chamfer_fwd_ws.
 * VPN_E_TOOBIG if K > 64, the image has more than 16384 tiles or the rider's scratch (84 K + 4 (K + 2) + tiles bytes) does
 * not fit the scan's 24 KB of LDS (the caller then runs without it).  vpn_hotpath_tile_rider_fits: 1 if the rider is taken
 * for (K, H, W), 0 if that is the answer; host arithmetic only, no HIP call. */
size_t vpn_raster_order_size(int B, int H, int W);
int vpn_hotpath_tile_rider_fits(int K, int H, int W);
int vpn_hotpath_chamfer_fwd(const float* p1, const float* p2, int B, int N, int M, float* dist1, int32_t* idx1,
                            float* dist2, int32_t* idx2, void* workspace, size_t workspace_bytes, int mode,
                            void* records, int K, int H, int W, void* tile_order, void* stream);
int vpn_loss_finalize(void* loss_ws, int B, int H, int W, const float* dist1, const float* dist2, int N, int M,
                      float cd_w1, float cd_w2, float w_cd, float w_sil, float w_dep, float* losses, float* loss_b,
                      void* stream);
int vpn_raster_total_bwd(const float* params, const float* cam, int B, int K, int H, int W,
                         const void* records, const void* workspace, const float* grad_total,
                         float* grad_params, int accumulate, void* stream);
/* Backward of the whole training step in ONE launch: vpn_sample_chamfer_bwd and vpn_raster_total_bwd together
 * (both are one workgroup per (sample, primitive)):
 *   grad_params = d(Chamfer term)/d params [as vpn_sample_chamfer_bwd] + (*grad_total) * d(total_img)/d params.
 * grad_loss_b may be NULL: then d total / d loss_b = *grad_total for every sample, and the caller folds the constant
 * factors of the batch mean into the weights (w1 = cd_w1 * w_cd / B, w2 = cd_w2 * w_cd / B): no kernel in between. */
int vpn_hotpath_bwd(const float* params, const int32_t* kinds, const float* u,
                    uint64_t seed, const uint64_t* seed_dev, uint64_t sample_base, int B, int K, int n,
                    const float* points, const float* gt_points, int M,
                    const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2,
                    const float* grad_loss_b, float w1, float w2,
                    const float* cam, int H, int W, const void* records, const void* workspace,
                    const float* grad_total, float* grad_params, void* stream);

/* ---- fused camera transforms (row f3): view_to_obj_points / obj_to_view_points
 * (modules/transform/transform.py:21-47, :50-73; called on train.py:158 every step).
 * points [B,N,3]; dists, elevs, azims, angles [B] (degrees, as the reference's callers pass them; angles may
 * be NULL when to_object == 0).  to_object != 0: out = dist * R(-z,-e) R(y',-a) R(x,-angle) p;
 * to_object == 0: out = R(y',a) R(-z,e) p / dist.  One launch instead of 3-4 rotate_points + a scale.
 * The camera is data (dataset.py:145-165): only the points receive a gradient. */
int vpn_camera_transform_fwd(const float* points, const float* dists, const float* elevs, const float* azims,
                             const float* angles, int B, int N, int to_object, float* out, void* stream);
int vpn_camera_transform_bwd(const float* grad_out, const float* dists, const float* elevs, const float* azims,
                             const float* angles, int B, int N, int to_object, float* grad_points, void* stream);

/* ---- primitive -> mesh vertices (row f2: modules/meshing/sphere.py:8-27, cuboid.py:8-26, meshing.py:27-46)
 * verts [B, Ptot, 3]: verts[b][offsets[k] + p] = R(q_bk) (tpl[p] * v_bk) + t_bk, tpl = tpl_sphere [Ps,3] or
 * tpl_cuboid [Pc,3] by kinds[k]; offsets [K+1] int32 (device): vertex offsets of the composed mesh, offsets[K] = Ptot.
 * The reference parses the OBJ template from disk per (sample, primitive); here the templates are device arrays the
 * caller keeps (a template of a kind that does not occur may be NULL). */
int vpn_mesh_fwd(const float* params, const int32_t* kinds, const int32_t* offsets,
                 const float* tpl_sphere, const float* tpl_cuboid, int B, int K, int Ptot, float* verts, void* stream);
int vpn_mesh_bwd(const float* params, const int32_t* kinds, const int32_t* offsets,
                 const float* tpl_sphere, const float* tpl_cuboid, int B, int K, int Ptot,
                 const float* grad_verts, float* grad_params, void* stream);

/* ---- the triangle-mesh path: meshes that carry NO primitives (train_sphere.py:53-76,128: the 386-vertex sphere of
 * 386.obj deformed in place, sampled by kaolin's TriangleMesh.sample and rendered by VertexRenderer.render /
 * SilhouetteLoss.forward through kaolin's DIBRenderer, vertex_renderer.py:20-24).  kaolin is absent: the arithmetic is
 * this repository's specification (oracle.vpn_oracle.mesh_raster / mesh_sample), parity unpinned.
 * verts [B,P,3] fp32 (B meshes of one topology), faces [F,3] int32 (vertex indices, clamped to [0,P) on the device),
 * cam [B,3] = (dist, elev deg, azim deg) as vpn_raster_fwd.
 * vpn_mesh_raster_fwd: alpha [B,H,W] = 1 - prod_f (1 - sigmoid(+-d2_f / sigma)), d2_f = squared NDC distance of the
 *   pixel centre to the nearest edge of face f, + inside / - outside; workspace = vpn_mesh_raster_workspace(B, P) bytes
 *   (projected vertices, kept for the backward call).
 * vpn_mesh_raster_bwd: grad_verts [B,P,3] = d (sum grad_alpha . alpha) / d verts (same workspace as the forward call).
 * vpn_mesh_sample_fwd: n area-weighted uniform surface points per mesh: points [B,n,3], face_idx [B,n], bary [B,n,3]
 *   (the barycentric weights, for the backward); u [B,n,3] explicit uniforms or NULL = Philox(seed; mesh_base + b,
 *   slot 0xFFFFFFFF, point); cdf [B,F] scratch (cumulative face areas).
 * vpn_mesh_sample_bwd: grad_verts [B,P,3] = sum_i bary_i * grad_points_i (the face choice is not differentiated). */
size_t vpn_mesh_raster_workspace(int B, int P);
int vpn_mesh_raster_fwd(const float* verts, const int32_t* faces, const float* cam, int B, int P, int F, int H, int W,
                        float sigma, void* workspace, float* alpha, void* stream);
int vpn_mesh_raster_bwd(const float* verts, const int32_t* faces, const float* cam, int B, int P, int F, int H, int W,
                        float sigma, void* workspace, const float* alpha, const float* grad_alpha, float* grad_verts,
                        void* stream);
int vpn_mesh_sample_fwd(const float* verts, const int32_t* faces, const float* u, uint64_t seed, uint64_t mesh_base,
                        int B, int P, int F, int n, float* cdf, float* points, int32_t* face_idx, float* bary, void* stream);
int vpn_mesh_sample_bwd(const int32_t* faces, const int32_t* face_idx, const float* bary, const float* grad_points,
                        int B, int P, int F, int n, float* grad_verts, void* stream);

/* ---- head post-processing into packed primitive parameters (row f4)
 * restrict_range + split + restrict_volumes of the reference's model (modules/network/vpnet_one_resnet.py:34-41,
 * :67-85): volumes [B,3K], rotates [B,4K], translates [B,3K] (raw head outputs) -> params [B,K,10].
 * is_sigmoid != 0 (config.py:25): v = (sigmoid(x) + 0.1) / restrict[j], q = sigmoid(x), t = tanh(x);
 * else v = clamp(x, clamp_min + 1e-8, clamp_max) / restrict[j], q, t = clamp(x, -1, 1) (config.py:22-23, :26). */
int vpn_head_pack_fwd(const float* volumes, const float* rotates, const float* translates, int B, int K,
                      int is_sigmoid, float clamp_min, float clamp_max, float restrict0, float restrict1,
                      float restrict2, float* params, void* stream);
/* grad_params [B,K,10] -> gradients of the raw head outputs (any of the three may be NULL). */
int vpn_head_pack_bwd(const float* volumes, const float* rotates, const float* translates, const float* grad_params,
                      int B, int K, int is_sigmoid, float clamp_min, float clamp_max, float restrict0,
                      float restrict1, float restrict2, float* grad_volumes, float* grad_rotates,
                      float* grad_translates, void* stream);

/* ---- the reference's whole training step (train.py:243-262) around the hot path: BASELINE config C5
 *   total = L_VIEW_CD * ChamferDistanceLoss(pred, view_center)            (train.py:160)   [vpn_hotpath_*]
 *         + L_CAN_CD  * ChamferDistanceLoss(view_to_obj(pred), canonical) (train.py:158-161)
 *         + L_SIL     * SilhouetteLoss(primitives, silhouettes)           (train.py:176)   [vpn_raster_total_fwd_fin]
 *         + L_VP_DIV  * VPDiverseLoss(translates, view_center)            (train.py:185, vp_diverse.py:12-18)
 *         + L_EMD     * sqrt(EMD dist).mean()                             (train.py:193-195) [vpn_emd_fwd]
 * vpn_vpdiv_fwd: the nearest neighbours of VPDiverseLoss -- centres = params[b,k,7:10] (the reference cats the K
 *   translations), both directions: dist1/idx1 [B,K] (centre -> nearest ground-truth point), dist2/idx2 [B,M]; same
 *   arithmetic and tie rule as vpn_chamfer_fwd (chamfer_distance.py:14-23).  dist1 = idx1 = NULL: the centres' direction stays
 *   as per-slice results in `workspace` for vpn_trainstep_finalize to merge.
 * vpn_camera_matrix: mat [B,9] row-major with view_to_obj_points(p) = mat p (to_object != 0; transform.py:21-47) or
 *   obj_to_view_points(p) = mat p (to_object == 0; :50-73), the scale by dist included.
 * vpn_trainstep_finalize: out [6] = (L_VIEW_CD*view_cd, L_CAN_CD*obj_cd, L_SIL*sil, L_VP_DIV*vp_div, L_EMD*emd, their sum)
 *   from hot_losses [4] as vpn_raster_total_fwd_fin leaves them (w_cd = L_VIEW_CD, w_sil = L_SIL, w_dep = 0), the
 *   auction's dist [B,N], the object-centred cloud's nearest-neighbour distances cn_dist1 [B,N] / cn_dist2 [B,Mc] and
 *   the VP-diversity distances dv_dist1 [B,K] / dv_dist2 [B,M]; any of the three groups may be NULL (term = 0).
 *   Fixed summation order.  dv_workspace != NULL (then dv_dist1 == NULL): the workspace a preceding vpn_vpdiv_fwd call
 *   with dist1 = idx1 = NULL left its per-slice results in; they are merged into dv_dist1_out / dv_idx1_out [B,K] by the
 *   same per-sample pass (one launch less in the training step).
 * vpn_trainstep_bwd: grad_params [B,K,10] = (*grad_total) * d total / d params in ONE launch: vpn_hotpath_bwd (w1 =
 *   cd_w1 * L_VIEW_CD / B, w2 = cd_w2 * L_VIEW_CD / B; records / workspace NULL when the silhouette term is off) plus
 *   - the EMD term through the assignment (emd_cuda.cu:284-300 and the sqrt / mean of train.py:195): emd_coef = L_EMD / (B N);
 *   - the VP-diversity term, straight into the translations: dv_c1 = L_VP_DIV * 0.5 / (K B), dv_c2 = L_VP_DIV * 1.0 / (M B);
 *   - the object-centred Chamfer term through cn_mat [B,9] (cn_points = the transformed cloud, cn_gt [B,cn_M,3],
 *     its four nearest-neighbour arrays): cn_c1 = L_CAN_CD * cd_w1 / (N B), cn_c2 = L_CAN_CD * cd_w2 / (cn_M B).
 *   A group whose first pointer is NULL is skipped (the reference's default L_CAN_CD = 0 multiplies that gradient by 0). */
size_t vpn_vpdiv_workspace(int B, int K);          /* scratch of vpn_vpdiv_fwd (8-byte aligned) */
int vpn_vpdiv_fwd(const float* params, const float* gt_points, int B, int K, int M, float* dist1, int32_t* idx1,
                  float* dist2, int32_t* idx2, void* workspace, void* stream);
int vpn_camera_matrix(const float* dists, const float* elevs, const float* azims, const float* angles, int B,
                      int to_object, float* mat, void* stream);
size_t vpn_trainstep_workspace(int B);             /* scratch of vpn_trainstep_finalize (per-sample sums) */
int vpn_trainstep_finalize(const float* hot_losses, const float* emd_dist, const float* cn_dist1, const float* cn_dist2,
                           const float* dv_dist1, const float* dv_dist2, int B, int N, int M, int Mc, int K,
                           float w_view, float w_can, float w_sil, float w_div, float w_emd, float cd_w1, float cd_w2,
                           void* workspace, const void* dv_workspace, float* dv_dist1_out, int32_t* dv_idx1_out,
                           float* out, void* stream);
int vpn_trainstep_bwd(const float* params, const int32_t* kinds, uint64_t seed, const uint64_t* seed_dev,
                      uint64_t sample_base, int B, int K, int n, const float* points, const float* gt_points, int M,
                      const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2,
                      float w1, float w2, const float* cam, int H, int W, const void* records,
                      const void* workspace, const float* grad_total,
                      const float* emd_dist, const int32_t* emd_assign, float emd_coef,
                      const float* dv_dist1, const int32_t* dv_idx1, const float* dv_dist2, const int32_t* dv_idx2,
                      float dv_c1, float dv_c2,
                      const float* cn_points, const float* cn_gt, const float* cn_mat, const float* cn_dist1,
                      const int32_t* cn_idx1, const float* cn_dist2, const int32_t* cn_idx2, float cn_c1, float cn_c2,
                      int cn_M, float* grad_params, void* stream);

/* ---- Earth Mover's Distance, auction approximation (row f1)
 * Replaces emd.forward / emd.backward of the reference's CUDA extension (modules/loss/emd/emd_cuda.cu:228-282,
 * :302-316, bound in emd_module.py:56, :69).  xyz1, xyz2 [B,n,3] (the reference requires equal sizes,
 * emd_module.py:36); dist [B,n] = squared distance of every xyz1 point to its assigned xyz2 point;
 * assignment [B,n] int32.  The nine scratch tensors the reference's caller allocates (emd_module.py:44-54)
 * become one workspace of vpn_emd_workspace(B, n) bytes.  iters >= 1, eps >= 0.  n need not be a multiple
 * of 1024 and B is not limited to 512 (emd_module.py:38-39). */
/* max_group: cap on the number of workgroups that cooperate on one sample (0 = automatic: as many as can be
 * resident together by hipOccupancyMaxActiveBlocksPerMultiprocessor x #CU, power of two <= 16; 1 = one workgroup per
 * sample, nothing shared between workgroups).  Co-residency: the workgroups of a sample wait for each other's bids, so
 * they must all be resident together.  The occupancy bound guarantees that for a plain launch on a GPU that runs nothing
 * else at the time; when other processes or streams share the GPU (several ranks on one device, a long kernel of another
 * stream) some may not be.  Their wait is bounded (~0.5 s), the sample is flagged, and every call that ran with G > 1
 * ends with a second launch at G = 1 on the same stream that recomputes the flagged samples: the result is always the
 * G = 1 result, with no host synchronisation (the call stays capturable in a HIP graph).  On an idle GPU that launch is one
 * wave of workgroups that read their flag and leave.  Sharing the GPU therefore costs time (the spin, then the redo),
 * never correctness; max_group = 1 avoids the cost where sharing is the rule.  VPN_EMD_COOP_LAUNCH=1 in the environment launches cooperatively (the runtime then checks
 * residency itself; the call falls back to 1 if it refuses) -- not the default: a cooperative launch in a process that has
 * captured a HIP graph slows every later dispatch of that process by ~50 us.  Results do not depend on any of this.
 * For 128 <= n <= 2048 the auction is one workgroup per CU (1024 threads, <= 128 VGPRs, 131 KB of LDS at n = 2048,
 * G = 4 at B = 64): kernels of ANOTHER stream that need <= 32 KB of LDS and <= 4 waves per SIMD run beside it, which is
 * how TrainStepLossFunction uses it -- launch the auction first, so its workgroups are placed while the CUs are empty (a
 * workgroup that must wait for a slot only makes its partners spin, bounded as above).  Environment, performance only:
 * VPN_EMD_FORM=team|local|streaming (the kernel; by default team for 128 <= n <= 2048, local for other n <= 4096,
 * streaming above; an override is ignored where its kernel cannot take n),
 * VPN_EMD_FLAT_MIN (default 1: own bidders from which a round after the first bids in the balanced form; 0 = team
 * form only), VPN_EMD_FLAT_WORK (default 0: own bidders x targets per bid of the last balanced round from which it
 * does), VPN_EMD_TNUM / VPN_EMD_TMAX (default 1024 / 16: lanes a round's own bidders are spread over / largest team),
 * VPN_EMD_COOP_LAUNCH (above). */
size_t vpn_emd_workspace(int B, int n);
int vpn_emd_fwd(const float* xyz1, const float* xyz2, int B, int n, float eps, int iters,
                float* dist, int32_t* assignment, void* workspace, int max_group, void* stream);
/* vpn_emd_fwd with a test hook (vpn_emd_fwd passes 0): a sample b < 32 with bit b of test_giveup_mask set gives up at its
 * first group barrier at once when G > 1 (no spin, no wait), as if its workgroups could not all be resident, so that
 * the recovery above runs deterministically.  The result does not change. */
int vpn_emd_fwd_ex(const float* xyz1, const float* xyz2, int B, int n, float eps, int iters,
                   float* dist, int32_t* assignment, void* workspace, int max_group, void* stream,
                   unsigned test_giveup_mask);
/* Samples the G = 1 recovery launches have recomputed on the current device since the library was loaded.  Waits for
 * the device (hipDeviceSynchronize): call it between steps, not inside one.  < 0: -(HIP error). */
long long vpn_emd_recovered_samples(void);
/* Workgroups per sample (G) of the last vpn_emd_fwd / vpn_emd_fwd_ex launch in this process (0: none yet). */
int vpn_emd_last_group(void);
/* grad_xyz1 [B,n,3] = 2 grad_dist (xyz1 - xyz2[assignment]) is written; xyz2 receives no gradient
 * (emd_module.py:66-70 returns zeros for it). */
int vpn_emd_bwd(const float* xyz1, const float* xyz2, const float* grad_dist, const int32_t* assignment,
                int B, int n, float* grad_xyz1, void* stream);

/* ---- the GCN refinement stage (modules/network/gcn.py, GCNModel; train_gcn.py / test_gcn.py)
 * vpn_gcn_aggregate: out [B,N,C] = A x [B,N,C] + bias [C] (bias may be NULL), then max(., 0) when relu != 0, where A is a
 *   CSR matrix over the N vertices (row_ptr [N+1], col / w [nnz]; the GCN uses the symmetric A = D^-1/2 (A_mesh + I)
 *   D^-1/2 of PyG's gcn_norm).  mask != NULL ([B,N,C]): x[j] counts only where mask[j] > 0 (the backward of a ReLU'd
 *   layer: dx = A (g * [y > 0]) for symmetric A).  Fixed summation order (CSR order), no atomics.
 * vpn_gcn_colsum: out [S,C] = sum_{r < R} in[(s R + r) ld + off + c] (* [mask > 0], mask indexed like in, may be NULL) in
 *   a fixed order; workspace of vpn_gcn_colsum_workspace(S, R, C) bytes.
 * vpn_gcn_bounds: get_bound_of_images (gcn.py:90-133) of img [B,C,H,W] -> bounds [B,4] in [-1,1], bit-exact: mask =
 *   sum_c img > 0.03 (channels added in order); b0 = min{i >= 1 : column i occupied} else 0, b1 = max{j : column j
 *   occupied} else W, rows alike; b / W * 2 - 1, b / H * 2 - 1 in fp32.
 * vpn_gcn_input_fwd: conv1's input out [B,N,venc + sum C_l + G] = [encoding | pooled | global] (gcn.py:36-42) of verts
 *   [B,N,3]: venc = 0 (none), 3 (the vertices) or 39 (positional encoding [x, sin x, cos x, sin 2x, ..., cos 32x],
 *   gcn.py:73-82); pooled = bilinear samples (align_corners, zero padding, as grid_sample) of the L <= 4 NCHW maps f_l
 *   [B,C_l,H_l,W_l] at the grid of gcn.py:141-153 (per-sample min / max of z and y, bounds [B,4]); global [B,G] repeated
 *   (G may be 0).  Writes ext [B,4] (zmin, zmax, ymin, ymax), ext_idx [B,4] (their first vertex), grid [B,N,2] and the
 *   NHWC copy of the maps in maps_ws (vpn_gcn_maps_workspace bytes); the backward reads all four.  With L = 0 bounds,
 *   ext, ext_idx, grid and maps_ws may be NULL.  zmax == zmin or ymax == ymin divides by zero, as the reference does.
 * vpn_gcn_input_bwd: from grad [B,N,ctot]: grad_verts [B,N,3] (NULL: skipped) through the encoding, the grid and the
 *   min / max (to the first arg-extreme vertex), and the map gradients gf_l [B,C_l,H_l,W_l] (all NULL: skipped), summed
 *   per pixel over the vertices sorted by bilinear cell: deterministic, no atomics; N <= 8192 then.  The gradient of the
 *   global block is a column sum (vpn_gcn_colsum).  workspace: vpn_gcn_input_bwd_workspace bytes. */
int vpn_gcn_aggregate(const float* x, const int32_t* row_ptr, const int32_t* col, const float* w, const float* bias,
                      const float* mask, int B, int N, int C, int relu, float* out, void* stream);
size_t vpn_gcn_colsum_workspace(int S, int R, int C);
int vpn_gcn_colsum(const float* in, const float* mask, int S, int R, int ld, int off, int C, void* workspace, float* out,
                   void* stream);
int vpn_gcn_bounds(const float* img, int B, int C, int H, int W, float* bounds, void* stream);
size_t vpn_gcn_maps_workspace(int B, int L, int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2, int W2,
                              int C3, int H3, int W3);
int vpn_gcn_input_fwd(const float* verts, const float* bounds, const float* global_features, int B, int N, int G,
                      int venc, int L, const float* f0, const float* f1, const float* f2, const float* f3, int C0,
                      int H0, int W0, int C1, int H1, int W1, int C2, int H2, int W2, int C3, int H3, int W3,
                      float* ext, int32_t* ext_idx, float* grid, void* maps_ws, float* out, void* stream);
size_t vpn_gcn_input_bwd_workspace(int B, int N, int L, int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2,
                                   int W2, int C3, int H3, int W3);
int vpn_gcn_input_bwd(const float* grad, const float* verts, const float* bounds, int B, int N, int G, int venc, int L,
                      int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2, int W2, int C3, int H3, int W3,
                      const float* ext, const int32_t* ext_idx, const float* grid, const void* maps_ws,
                      void* workspace, float* grad_verts, float* gf0, float* gf1, float* gf2, float* gf3,
                      void* stream);

/* ---- conv1 of the GCN in factored form: h = [encoding | pooled | global] Theta without the row.
 * Theta [venc + sum C_l + G, Cout] splits row-wise into Theta_e, Theta_l, Theta_g.  The caller projects the maps, proj
 * [B, sum H_l W_l, Cout] = map_l (NHWC) Theta_l level after level (vpn_gcn_factored_proj_workspace bytes), and the global
 * features, gtheta [B,Cout] = g Theta_g (NULL: no global block); theta_e [venc,Cout] are Theta's first rows (NULL with
 * venc = 0).  Cout % 4 == 0; out, proj, gtheta and theta_e are 16-byte aligned.
 * vpn_gcn_factored_fwd: out [B,N,Cout] = sum_k enc_k(v) Theta_e[k] + sum_l sum_corner w proj_l[b,pix] + gtheta[b], summed
 *   in that order (corners nw, ne, sw, se) with the grid, corner, weight and validity rules of vpn_gcn_input_fwd; writes
 *   ext, ext_idx and grid like it (NULL allowed with L = 0).
 * vpn_gcn_factored_bwd: from grad [B,N,Cout], each skipped when its pointer is NULL: grad_proj [B, sum H_l W_l, Cout] (per
 *   pixel the weighted sum of grad over the vertices touching it, sorted by cell as in vpn_gcn_input_bwd; N <= 8192),
 *   grad_theta_e [venc,Cout] = sum_{b,v} enc_k(v) grad (partial sums over 128 rows, then those in order) and grad_verts
 *   [B,N,3] through the encoding (grad Theta_e^T), the grid and the min / max.  No atomics.  The gradients of Theta_l,
 *   Theta_g, the maps and the global features are dense products of grad_proj and the column sum of grad with the
 *   caller's tensors.  workspace: vpn_gcn_factored_bwd_workspace bytes. */
size_t vpn_gcn_factored_proj_workspace(int B, int Cout, int L, int H0, int W0, int H1, int W1, int H2, int W2, int H3,
                                       int W3);
int vpn_gcn_factored_fwd(const float* verts, const float* bounds, const float* gtheta, const float* theta_e,
                         const float* proj, int B, int N, int Cout, int venc, int L, int H0, int W0, int H1, int W1,
                         int H2, int W2, int H3, int W3, float* ext, int32_t* ext_idx, float* grid, float* out,
                         void* stream);
size_t vpn_gcn_factored_bwd_workspace(int B, int N, int Cout, int venc, int L, int H0, int W0, int H1, int W1, int H2,
                                      int W2, int H3, int W3);
int vpn_gcn_factored_bwd(const float* grad, const float* verts, const float* bounds, const float* theta_e,
                         const float* proj, int B, int N, int Cout, int venc, int L, int H0, int W0, int H1, int W1,
                         int H2, int W2, int H3, int W3, const float* ext, const int32_t* ext_idx, const float* grid,
                         void* workspace, float* grad_verts, float* grad_proj, float* grad_theta_e, void* stream);

/* ---- the GCN's layer pairs as one linear map each (csrc/gcnpair.hip).
 * vpn_gcn_aggregate2: out [B,N,C] = A( A h + 1 (x) u ) + 1 (x) bias, then max(., 0) when relu != 0; u and bias [C] may be
 *   NULL.  A in CSR form as for vpn_gcn_aggregate.  blocks [nblocks + 1] int32: ascending starts of index ranges of at
 *   most 128 rows that cover [0, N) and that no entry of A crosses (blocks[0] = 0, blocks[nblocks] = N); both hops of a
 *   range run in LDS.  An entry that leaves its range is not added; a range that is empty, longer than 128 or outside
 *   [0, N] is not computed.  Each hop sums a row in CSR order as vpn_gcn_aggregate does and the intermediate is rounded
 *   to fp32: out equals two calls of vpn_gcn_aggregate bit for bit.  mask != NULL ([B,N,C]): h counts only where mask > 0
 *   (the backward of a ReLU'd pair: out = the gradient of h).  du_partial != NULL ([B, nblocks, C],
 *   vpn_gcn_aggregate2_workspace bytes): the sum over each range's rows, in row order, of the intermediate A h + u; its
 *   column sum over (b, range) is the gradient of u when the call is a backward.  No atomics.
 * vpn_gcn_project_fwd: out [R,Co] = x [R,Ci] theta [Ci,Co] for Co <= 4 and Ci <= 1024, every result the fixed-order sum of
 *   a wave.  vpn_gcn_project_bwd: dx [R,Ci] = grad theta^T (NULL: skipped) and dtheta [Ci,Co] = x^T grad (NULL: skipped)
 *   as partial sums over 64-row chunks (workspace: vpn_gcn_project_bwd_workspace bytes) added in chunk order.  No atomics. */
size_t vpn_gcn_aggregate2_workspace(int B, int nblocks, int C);
int vpn_gcn_aggregate2(const float* h, const float* mask, const int32_t* row_ptr, const int32_t* col, const float* w,
                       const int32_t* blocks, int nblocks, const float* u, const float* bias, int B, int N, int C,
                       int relu, float* out, float* du_partial, void* stream);
size_t vpn_gcn_project_bwd_workspace(int R, int Ci, int Co);
int vpn_gcn_project_fwd(const float* x, const float* theta, int R, int Ci, int Co, float* out, void* stream);
int vpn_gcn_project_bwd(const float* grad, const float* x, const float* theta, int R, int Ci, int Co, void* workspace,
                        float* dx, float* dtheta, void* stream);

/* ---- the batch augmentation stage (train.py:232-237): CutMix and the point mix-up.  Outputs are data: no backward.
 * vpn_cutmix_points: cut_mix_batch_points + adjust_point_num (modules/augmentation/cutmix.py:24-50).  points [B,N,3];
 *   indices [B] = the partner of each sample (NULL: every sample is its own partner; a value outside [0,B) is read as
 *   the sample itself); the cut is cut_per_sample[b] when that pointer is not NULL, else `cut`.  The 2 N candidates of
 *   sample b are numbered 0..N-1 (its own points) and N..2N-1 (its partner's); the eligible list is the reference's
 *   cat([own[z >= cut], partner[z < cut]]) (cutmix.py:32) in that order.  out [B,n_out,3], src [B,n_out], count [B]:
 *     count == n_out: the eligible list in order;
 *     count >  n_out: n_out distinct members, every n_out-subset equally likely (randperm(count)[:n_out], :46), in the
 *                     order of the draw;
 *     0 < count < n_out: n_out independent uniform draws (randint(0, count, (n_out,)), :49);
 *     count == 0: src[b,i] = i mod N, the sample's own points.  THE ONE DEVIATION: the reference raises here (randint(0, 0):
 *                 "from >= to"), which needs a host synchronisation; count[b] = 0 tells the caller instead.
 *   out[b,i] is candidate src[b,i] bit for bit.  The reference passes n_out = N; adjust_point_num alone is B = 1,
 *   indices = NULL, cut = -inf.  Draws are Philox4x32-10 words keyed on (seed, sample_base + b, slot) as the sampler's
 *   are, so a shard of a batch draws what the whole batch would.  One workgroup per sample, vpn_cutmix_points_lds(N)
 *   bytes of LDS; N > VPN_CUTMIX_MAX_POINTS is VPN_E_TOOBIG before anything is launched (vpn_cutmix_points_lds: 0).
 * vpn_cutmix_images: cutmix.py:17-18 for two images in one launch: out[b,c,y,x] = x < cut_index ? img[b,c,y,x] :
 *   img[indices[b],c,y,x] for img_a [B,Ca,H,W] and img_b [B,Cb,H,W] (Cb = 0: img_b / out_b unused), 0 <= cut_index <= W.
 *   Out of place: out_* must not overlap img_*.  16-byte accesses when W % 4 == 0 and the four pointers are 16-byte
 *   aligned, element-wise otherwise.
 * vpn_mixup_gather: out [B,n,3] = points[indices[b]] (point_mixup.py:32-33, for the whole batch).
 * vpn_mixup_lerp: out[b,i] = wa * points[b,i] + wb * partner[b, assignment[b,i]] (point_mixup.py:36-37), each product and
 *   the sum rounded by itself; assignment [B,n] is vpn_emd_fwd's (points vs partner); an entry outside [0,n) leaves the
 *   point where it is. */
size_t vpn_cutmix_points_lds(int N);
int vpn_cutmix_points(const float* points, const int32_t* indices, const float* cut_per_sample, float cut, uint64_t seed,
                      uint64_t sample_base, int B, int N, int n_out, float* out, int32_t* src, int32_t* count,
                      void* stream);
int vpn_cutmix_images(const float* img_a, const float* img_b, const int32_t* indices, int B, int Ca, int Cb, int H, int W,
                      int cut_index, float* out_a, float* out_b, void* stream);
int vpn_mixup_gather(const float* points, const int32_t* indices, int B, int n, float* out, void* stream);
int vpn_mixup_lerp(const float* points, const float* partner, const int32_t* assignment, int B, int n, float wa, float wb,
                   float* out, void* stream);

/* ---- the evaluation stage (test.py:68-135, test_gcn.py:115-178): per-sample metrics of a batch and the per-class
 * bookkeeping of an evaluation epoch on the device.  One launch per batch replaces the last reduction of
 * ChamferDistanceLoss(each_batch=True) (chamfer_distance.py:25-30, called at test.py:101 / test_gcn.py:89), torch.sqrt(dist)
 * .mean(1) (test_gcn.py:83), the two batch means with their .item() (test.py:104, test_gcn.py:145-146) and the class loop
 * with its 2 B .item() calls (test.py:105-107, test_gcn.py:149-152).
 * state: vpn_eval_state_size(C) bytes, 8-byte aligned, ZEROED BY THE CALLER before the first batch of an epoch (there is no
 *   reset entry point), then owned by the launches.  Layout, for C = num_classes: 3 + 2 C doubles
 *     [0] total_cd = sum over batches of mean_b cd_b     [1] total_emd likewise
 *     [2] the arrival ticket of the launch in flight, an int in an 8-byte slot: 0 between launches (reads as 0.0)
 *     [3, 3+C) class_sum_cd     [3+C, 3+2C) class_sum_emd
 *   followed by 2 + C int64:  [0] n_batches   [1] n_invalid   [2, 2+C) class_n.
 *   Two states are merged by adding them field by field (ranks that each evaluated a shard).
 * vpn_eval_accumulate: dist1 [B,N] / dist2 [B,M] = the nearest-neighbour distances of vpn_chamfer_fwd*; emd_dist [B,N] =
 *   the auction's dist (needs N == M), or NULL: Chamfer only, the test.py form (emd_b unused, the EMD fields keep their
 *   value); class_index [B] int32 on the device.  Writes
 *     cd_b[b]  = cd_scale * (w1 mean_i dist1[b,i] + w2 mean_j dist2[b,j]): the bits of vpn_chamfer_loss (one shared
 *                summation order), times cd_scale in fp32 (test.py:101 multiplies by L_VIEW_CD);
 *     emd_b[b] = mean_i sqrtf(emd_dist[b,i]), summed in fp64 in a fixed order and rounded to fp32 once;
 *   and then, by the workgroup that arrives last, in sample order b = 0 .. B-1 and in fp64 (what Python's `+= x.item()`
 *   does): class_sum_cd[c] += cd_b[b], class_sum_emd[c] += emd_b[b], class_n[c] += 1 for c = class_index[b]; total_cd +=
 *   mean_b cd_b, total_emd += mean_b emd_b (the mean formed in fp64); n_batches += 1.  A class index outside [0, C) -- the
 *   reference raises IndexError or wraps a negative one, which needs a host synchronisation -- is left out of the class
 *   sums and counted in n_invalid; its sample still enters the batch means.  No floating-point atomics: bitwise
 *   reproducible.  The ticket is reset by the launch itself, so a captured launch can be replayed.  Launches on one state
 *   must be ordered (one stream). */
size_t vpn_eval_state_size(int num_classes);
int vpn_eval_accumulate(const float* dist1, const float* dist2, const float* emd_dist, const int32_t* class_index,
                        int B, int N, int M, int num_classes, float w1, float w2, float cd_scale, void* state,
                        float* cd_b, float* emd_b, void* stream);

/* ---- the visualisation stage (modules/visualize/render.py:13-24 as driven by vp_mesh.py:14-32,73-92 and mesh.py:7-50):
 * colour renders of V views of S samples in ONE launch, written as uint8 RGB (HWC) into a caller-owned frame buffer.  The
 * reference renders one view of one mesh per DIBRenderer call (13 to 37 per dump) and copies each to the host.
 * DIBRenderer is kaolin's: pixel values are parity-unpinned; the specification is DESIGN.md 4.10, restated by
 * tests/visualize_ref.py.  Forward only; plain launches on `stream`; no atomics; nothing is allocated.
 * cams [S,V,3] = (dist, elev deg, azim deg): the look-at camera of vpn_raster_fwd.  ambient in [0,1]: colour = base *
 *   (ambient + (1 - ambient) * cos(normal, ray)); 1 = flat colours, the reference's VertexColor look.  bg_*: background.
 * frames / frames_bytes / pitch / view_offset: pixel (row, col) of view (s, v) goes to
 *     frames + view_offset[s * V + v] + row * pitch + col * 3        (bytes; pitch >= 3 W)
 *   view_offset: S * V int64 on the device, or NULL for the dense layout [S,V,H,pitch].  A view whose rectangle leaves
 *   [0, frames_bytes) is skipped by the kernel (nothing of it is written); overlapping views are the caller's business.
 *   Quantisation: clamp to [0,1], times 255, truncate (torchvision's ToPILImage after a clamp).
 * vpn_vis_primitives (render.py:13-24 on primitives): params [S,K,10], kinds [K], palette [>= K,3] fp32.  Per pixel centre
 *   the ray eye + s (fwd + px right + py up) meets primitive k, in its scaled frame (o~, d~ of vpn_raster_fwd), at
 *     ellipsoid: hit iff 1 - m2 > 0, z = s* - sqrt((1 - m2) / (d~.d~))      cuboid: slab test on the unit box, hit iff
 *     t_near <= t_far, z = t_near (components |d~_i| < 1e-9 replaced as in the raster);
 *   a hit needs z > 1e-3; the nearest hit wins, equal depths go to the lowest k; no hit: background.  K <=
 *   VPN_VIS_MAX_PRIMS (VPN_E_TOOBIG beyond).
 * vpn_vis_mesh (render.py:13-24 on triangles): verts [S,P,3], faces [F,3] int32 shared by the samples, colors [S,P,3].
 *   workspace: vpn_vis_mesh_workspace(S, V, P) bytes, 16-byte aligned (the projected vertices; first launch).  Second
 *   launch: per pixel centre the faces that contain it (the inside rule of vpn_mesh_raster_fwd, faces with a corner at depth
 *   <= 1e-3 skipped, no back-face culling), depth and colour interpolated perspective-correctly, the nearest face wins,
 *   equal depths go to the lowest face; shading two-sided on the unit face normal. */
int vpn_vis_primitives(const float* params, const int32_t* kinds, const float* cams, const float* palette, int S, int K, int V,
                       int H, int W, float ambient, float bg_r, float bg_g, float bg_b, uint8_t* frames, size_t frames_bytes,
                       long long pitch, const long long* view_offset, void* stream);
size_t vpn_vis_mesh_workspace(int S, int V, int P);
int vpn_vis_mesh(const float* verts, const int32_t* faces, const float* colors, const float* cams, int S, int P, int F, int V,
                 int H, int W, float ambient, float bg_r, float bg_g, float bg_b, void* workspace, uint8_t* frames,
                 size_t frames_bytes, long long pitch, const long long* view_offset, void* stream);

/* ---- the Phong renderer (modules/render/phong_renderer.py:12-38 as driven by generate.py:150-161 and
 * point_mixup.py:58-70): textured, lit float renders of V views of S scenes of one topology.  The reference constructs a
 * DIBRenderer(mode='Phong') per view and copies each image to the host; DIBRenderer is kaolin's: pixel values are
 * parity-unpinned; the specification is DESIGN.md 4.11, restated by tests/phong_ref.py.  Forward only; plain
 * launches on `stream`; no atomics; nothing is allocated.  Added without a change of VPN_ABI_VERSION (entries
 * that are only added leave it).
 * vpn_phong_mesh: verts [S,P,3], faces [F,3] int32 shared by the scenes, uv [S,P,2], texture [S,3,TH,TW], cams [S,V,3] =
 *   (dist, elev deg, azim deg), light [3] in the camera basis (right, up, fwd), material [3,3] = rows ambient, diffuse,
 *   specular (RGB), all fp32 on the device; shininess >= 0.  workspace: vpn_phong_mesh_workspace(S, V, P) bytes, 16-byte
 *   aligned (the projected vertices; first launch).  Second launch: which face a pixel centre sees is the rule of
 *   vpn_vis_mesh (nearest face, equal depths to the lowest face, either winding, corners at depth <= 1e-3 skip the face);
 *   for that face (u, v) is interpolated perspective-correctly, tex = texture[s, :, clamp(floor(v TH)), clamp(floor(u TW))],
 *   n = the unit face normal turned towards the eye, l = the unit light, d = the unit pixel ray,
 *     cosT = clamp(n.l, 0, 1), r = 2 cosT n - l, cosA = clamp(-(r.d), 0, 1),
 *     rgb = clamp(tex * (ambient + diffuse * cosT) + specular * powf(cosA, shininess), 0, 1);
 *   a pixel that sees no face is (0, 0, 0).  rgb [S,V,H,W,3] fp32, every pixel written. */
size_t vpn_phong_mesh_workspace(int S, int V, int P);
int vpn_phong_mesh(const float* verts, const int32_t* faces, const float* uv, const float* texture, const float* cams,
                   const float* light, const float* material, float shininess, int S, int P, int F, int V, int TH, int TW,
                   int H, int W, void* workspace, float* rgb, void* stream);

/* ---- cloud -> mesh of one topology (the step of point_mixup.py:43-55 between mixup_points and the Phong
 * render).  The reference reconstructs a surface by ball pivoting (open3d, ball_pivot.py) and decomposes it with V-HACD
 * (trimesh + an external binary, convex_decomposition.py:7-16) per sample on the host; this REPLACES both: the cloud is
 * split into H clusters and every cluster becomes the polytope of its support points along D fixed directions, so all
 * samples share one face list.  Parity with the reference is unpinned; the specification is restated by
 * tests/reconstruct_ref.py and the outputs equal it bit for bit.  Forward only; plain launches on `stream`; nothing is
 * allocated.  Inputs must be finite (not checked on the device).  All fp32 arithmetic is rounded per operation, sums run
 * x, y, z from the left: dist2(p, c) = ((px-cx)^2 + (py-cy)^2) + (pz-cz)^2, dot(p, d) = (px dx + py dy) + pz dz.
 * n <= VPN_CLUSTER_MAX_POINTS, H <= VPN_CLUSTER_MAX_HULLS, B <= 65535: VPN_E_TOOBIG beyond, before any HIP call.  Added
 * without a change of VPN_ABI_VERSION.
 * Integer mean of a set: per coordinate sum llrint(x * 2^20) as int64 (exact in any order), (double)sum / ((double)count *
 *   2^20), rounded once to fp32.
 * vpn_cluster_points: points [B,n,3] -> labels [B,n] int32, centres [B,H,3], counts [B,H] int32; one workgroup per sample.
 *   Seeds: c_0 = the point with the largest dist2 to the integer mean of the cloud, c_k = the point with the largest
 *   min_j<k dist2(p, c_j); equal values go to the lowest point index.  Then `iters` >= 0 Lloyd rounds: every point takes the
 *   centre of smallest dist2 (equal values: the lowest centre), every non-empty cluster's centre becomes the integer mean
 *   of its members, an empty cluster keeps its centre.  labels and counts are one last assignment against the final
 *   centres.
 * vpn_support_hulls: labels / centres as above (a label outside [0,H) belongs to no cluster), dirs [D,3] ->
 *   verts [B,H*D,3], support [B,H*D] int32: vertex (h,d) is the member p of cluster h with the largest dot(p, dirs[d]),
 *   equal values to the lowest point index, support its index; an empty cluster writes its centre D times with support
 *   -1 (zero-area faces, which the raster and the sampler ignore).  One workgroup per (cluster, sample). */
int vpn_cluster_points(const float* points, int B, int n, int H, int iters, int32_t* labels, float* centres,
                       int32_t* counts, void* stream);
int vpn_support_hulls(const float* points, const int32_t* labels, const float* centres, const float* dirs, int B, int n,
                      int H, int D, float* verts, int32_t* support, void* stream);

/* ---- the middle of the ACD-mix stage (generate.py:140-148 with modules/augmentation/acd.py:31-77,114-119):
 * the hulls of the objects of a mix are augmented per object and merged.  The reference merges them with
 * trimesh.boolean.union (acd.py:105-111) on the host and decomposes the result again; this REPLACES the boolean by sampling
 * the surface of the union: candidates drawn on all augmented hulls survive unless they lie inside another kept hull, and
 * the surviving cloud is hulled again (vpn_cluster_points / vpn_support_hulls).  Parity with trimesh is unpinned; the
 * specification is restated by tests/acdmix_ref.py and the outputs equal it bit for bit.  Forward only; plain launches on
 * `stream`; no floating-point atomics; nothing is allocated.  Inputs must be finite (not checked on the device).  fp32
 * arithmetic is rounded per operation, dot(p, d) = (px dx + py dy) + pz dz.  G <= VPN_UNION_MAX_HULLS, D <=
 * VPN_UNION_MAX_DIRS, S <= VPN_UNION_MAX_SAMPLES, nc <= VPN_UNION_MAX_CAND: VPN_E_TOOBIG beyond, before any HIP call.  Added
 * without a change of VPN_ABI_VERSION.
 * vpn_hull_augment (acd.py:31-77,114-119): verts [S,G,D,3] = G hulls of D vertices per sample, group [G] int32 = the object
 *   a hull belongs to (0 .. O-1; for a mix of two objects of H hulls G = 2 H, O = 2; a hull with another value belongs to no
 *   object and is cut) -> out [S,G,D,3], keep [S,G] int32 (1 kept, 0 cut).  The draws of the reference come as data, per
 *   (sample, object) [S,O]: coin int32 (random.choice([True, False]), acd.py:70), u_num fp32 in [0,1) (for random.randint(1,
 *   |C|-1), :71), scale fp32 (:38), turn int32 0..4 indexing {90, -90, 0, 180, -180} degrees (:59; another value turns
 *   nothing), shift fp32 (:47); and per hull u_hull [S,G] fp32, the keys that stand for random.sample (:72).  One workgroup
 *   per (object, sample).
 *   is_center(h) (:31-34) = (some z > 0 and some z < 0) or some |z| < 0.05 over the D vertices of h as given.  With C the
 *   centre hulls of the object: if coin != 0 and |C| > 1, 1 + floor(u_num * (|C|-1)) hulls are cut, clamped to 1 .. |C|-1:
 *   those of C with the smallest u_hull, equal keys to the lowest hull index; every other hull of the object is kept (:73).
 *   Otherwise exactly C is kept (:75).  THE ONE DEVIATION: if C is empty all hulls of the object are kept (the reference
 *   goes on with an empty list and fails in the boolean).
 *   A kept hull gets, in the reference's order (:115-118): v *= scale; the turn about z; y += shift.  The turn is an exact
 *   signed swap: rotate_points with axis (0,0,1) multiplies by R = [[c,-s,0],[s,c,0],[0,0,1]] (rotate.py:23,36-44, angle / 360
 *   mod 1 turns, so -90 is 270 degrees): 90: (x,y) -> (-y,x); -90: (x,y) -> (y,-x); 0: unchanged; 180 and -180: (x,y) ->
 *   (-x,-y).  The reference's route through sinf / cosf of fp32 pi and a normalised quaternion gives these up to rounding
 *   (sin(pi) != 0 in fp32); the exact swap is what is specified here.  A cut hull collapses onto its first vertex as given
 *   (D copies): all its faces have zero area, which the mesh sampler and the rasters ignore.
 * vpn_union_surface: verts [S,G,D,3] and keep [S,G] as written above, dirs [D,3] the template's directions, cand [S,nc,3]
 *   candidates with cand_hull [S,nc] int32 = the hull a candidate was drawn on -> support [S,G,D], outside [S,nc] int32,
 *   points [S,n_out,3], src [S,n_out] int32, count [S] int32.  One workgroup per sample.
 *     support[h,d] = max_j dot(verts[h,j], dirs[d]) over the hull's own D vertices (the first of equal values), for every
 *       hull, cut or kept;
 *     p is outside h in direction d iff dot(p, dirs[d]) > support[h,d] - margin (the subtraction rounded to fp32); p is
 *       inside h iff no direction says outside;
 *     outside[c] = 1 iff candidate c's own hull is kept (cand_hull in [0,G) and keep != 0) and c is inside no other kept
 *       hull; count = the number of such candidates;
 *     points / src = the survivors in candidate order (stable compaction): slot i < count is survivor i, slot i >= count
 *       repeats survivor i mod count; count == 0 falls back to the candidates themselves, src[i] = i mod nc.
 *   points[s,i] is cand[s,src[s,i]] bit for bit.  margin: any finite fp32 (NaN is VPN_E_BADARG). */
int vpn_hull_augment(const float* verts, const int32_t* group, const int32_t* coin, const float* u_num, const float* scale,
                     const int32_t* turn, const float* shift, const float* u_hull, int S, int G, int D, int O, float* out,
                     int32_t* keep, void* stream);
int vpn_union_surface(const float* verts, const int32_t* keep, const float* dirs, const float* cand, const int32_t* cand_hull,
                      int S, int G, int D, int nc, int n_out, float margin, float* support, int32_t* outside, float* points,
                      int32_t* src, int32_t* count, void* stream);

/* ---- the image input stage (csrc/input.hip; modules/dataset/dataset.py:15-19,115-139 of the reference):
 * an RGBA rendering becomes the network input and the GT silhouette through PIL's Resize(BILINEAR), ColorJitter and
 * rotate(NEAREST), every pixel operation in PIL's own integer or per-operation-rounded fp32 arithmetic: the outputs equal
 * PIL's bit for bit (restated by tests/input_ref.py).  Forward only; three plain launches on `stream` (setup, resize,
 * finish); the only atomics are 64-bit integer adds (one sum per image, independent of their order); nothing is allocated.
 * Added without a change of VPN_ABI_VERSION.
 *   rgba [B,Hs,Ws,4] uint8 (R,G,B,A bytes, 4-byte aligned) -> inter [B,H,W,4] uint8, the resized image (Hs == H and
 *     Ws == W: a copy, as PIL); rgb [B,3,H,W], silhouette [B,1,H,W] fp32 = level / 255 (IEEE division) after jitter and
 *     rotation; angles_out [B] fp32 degrees, the angle each image was rotated by (0 without VPN_INPUT_ROTATE).
 *   tables: int32, hb [W,2] | hk [W,ksh] | vb [H,2] | vk [H,ksv]: for every output column / row the first source tap and
 *     the tap count, and the taps' coefficients round(k 2^22), built by the host in float64 as PIL's precompute_coeffs does.
 *     max_rows: the most source rows the vertical support of the VPN_INPUT_TILE_ROWS consecutive output rows of one tile
 *     spans (the LDS of one tile: 128 max_rows bytes <= 64 KB, VPN_E_TOOBIG beyond).  Entries that point outside the source are clamped on the device.
 *   flags: VPN_INPUT_JITTER | VPN_INPUT_ROTATE | VPN_INPUT_NORMALIZE (ImageNet mean / std, also on the rotation's zero fill).
 *   factors [B,3] fp32 (brightness, contrast, saturation), order [B,3] int32 (the operation of each turn: 0 brightness,
 *     1 contrast, 2 saturation), angles [B] fp32 degrees: the draws, each NULL or given.  A NULL one is drawn from
 *     Philox4x32-10, key seed + *seed_dev (seed_dev NULL or a DEVICE uint64, as vpn_sample_fwd), counter (slot, 0x80000001,
 *     sample_base + b): slot 0 gives u0..u3 = (word >> 8) 2^-24, factor_i = min(0.6 + 0.8 u_i, 1.4), angle = 360 u3 (360
 *     itself: 0); slot 1 gives the order, the (word * 6 >> 32)-th permutation in lexicographic order with Lemire's rejection.
 *   workspace: vpn_input_ws(B) bytes, 8-byte aligned (per image the L sum of the contrast mean and the fixed draws).
 *   All sides <= 8192, B <= 65535, B H W and B Hs Ws < 2^29: VPN_E_TOOBIG beyond, before any HIP call. */
#define VPN_INPUT_JITTER 1
#define VPN_INPUT_ROTATE 2
#define VPN_INPUT_NORMALIZE 4
#define VPN_INPUT_TILE_ROWS 8
size_t vpn_input_ws(int B);
int vpn_prepare_images(const uint8_t* rgba, const int32_t* tables, int ksh, int ksv, int max_rows, const float* factors,
                       const int32_t* order, const float* angles, uint64_t seed, const uint64_t* seed_dev,
                       uint64_t sample_base, int B, int Hs, int Ws, int H, int W, int flags, void* workspace,
                       size_t workspace_bytes, uint8_t* inter, float* rgb, float* silhouette, float* angles_out,
                       void* stream);

/* ---- the ground-truth stage (csrc/gtpoints.hip; modules/dataset/dataset.py:161-165 of the reference, called twice per item
 * at dataset.py:42-43, and genre.py:66-74): n area-weighted uniform surface points, T sets of them, on each
 * of S meshes of DIFFERENT sizes, all sets of a mesh from one cumulative-area table.  kaolin's TriangleMesh.sample is
 * absent: the result is this repository's specification (restated by tests/gtpoints_ref.py), parity
 * unpinned.  Forward only (ground truth is data); three plain launches on `stream` whatever S is; no atomics; nothing is
 * allocated; no host synchronisation.  Added without a change of VPN_ABI_VERSION.
 *   verts [sumP,3] fp32 and faces [sumF,3] int32: the meshes packed one after the other, vertex indices MESH-LOCAL (clamped
 *     to [0, P_s - 1] on the device); vert_offset / face_offset [S+1] int32: prefix sums of the vertex / face counts;
 *     chunks [C,3] int32 = (mesh, first face in the packed list, face count <= VPN_RAGGED_CHUNK), in face order, none
 *     straddling two meshes; chunk_offset [S+1] int32: the chunks of mesh s are [chunk_offset[s], chunk_offset[s+1]).
 *     Every offset is clamped into its array on the device.
 *   table: area_f = 0.5f * sqrtf(nx nx + ny ny + nz nz), n = (b - a) x (c - a), fp32, each operation rounded by itself;
 *     cum_f = the inclusive fp64 prefix sum of a mesh's areas in face order, rounded to fp32 where it is compared.
 *   draws: u [S,T,n,3] explicit uniforms, or NULL = Philox4x32-10, key seed + *seed_dev (seed_dev NULL or a DEVICE uint64),
 *     counter (point, 0xFFFFFFFF - set, mesh_base + s): set 0 draws what vpn_mesh_sample_fwd draws for that mesh index.
 *   face = the first whose (float)cum_f exceeds u0 * (float)cum_last, else the last; r = sqrtf(u1), bary = (1 - r,
 *     r (1 - u2), r u2), point = w0 a + w1 b + w2 c per component, left to right; xforms [S,T,3,4] (NULL: none): the point
 *     becomes row r: m[r][0] x + m[r][1] y + m[r][2] z + m[r][3], each product and sum rounded by itself, left to right,
 *     in the sets t whose bit of xform_mask is set (the other sets keep the point as it is, bit for bit).
 *   outputs: points [S,T,n,3]; face_idx [S,T,n] int32 (mesh-local) and bary [S,T,n,3], each may be NULL.
 *   workspace: vpn_ragged_sample_workspace(sumF, C, S) bytes, 16-byte aligned (the in-chunk prefix sums, the chunk bases,
 *     the mesh totals).
 *   T <= VPN_RAGGED_MAX_SETS, S T <= 65535, sumP and sumF <= INT32_MAX / 3: VPN_E_TOOBIG beyond, before any HIP call. */
size_t vpn_ragged_sample_workspace(int sumF, int C, int S);
int vpn_ragged_sample(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                      const int32_t* chunk_offset, const int32_t* chunks, const float* xforms, unsigned xform_mask, const float* u,
                      uint64_t seed, const uint64_t* seed_dev, uint64_t mesh_base, int S, int T, int n, int sumP, int sumF, int C,
                      void* workspace, size_t workspace_bytes, float* points, int32_t* face_idx, float* bary, void* stream);

/* ---- the network stage: the FC heads (csrc/fcstack.hip; modules/network/vpnet_one_resnet.py:31-41, :67-107,
 * vpnet_two_resnet.py:34-44, :70-110 and sdnet.py:19, :24-25, :41-50 of the reference): G groups of L
 * nn.Linear layers (the reference: 3 heads or SDNet's deform, 5 layers, 512 -> 1024 x 4 -> 3K | 4K | 3K) with nothing
 * between them but nn.Dropout, forward and backward.  Group g, layer l: y[b,o] = bias[o] + sum_i x[b,i] W[o,i], W in
 * nn.Linear's own [out,in] row-major layout; fp32 in, fp32 accumulate, summation order unspecified but fixed: outputs and
 * gradients are bit-equal from run to run (no float atomics).  One launch per layer forward, at most two per layer
 * backward, each covering all groups; plain launches on `stream`, nothing is allocated, no host synchronisation.
 * Added without a change of VPN_ABI_VERSION.
 *   VpnFcStack, passed BY VALUE (no device table): slot g * L + l belongs to layer l of group g, slot g alone to group g.
 *     x[g] [B,in0[g]]: the group's input (groups may share one); w / bias: the layer's parameters [out,in] / [out], where
 *     in = in0[g] for l = 0 and out[g * L + l - 1] otherwise; keep: uint8 [B,out] keep masks of layers 0..L-2 (read under
 *     VPN_FC_DROPOUT_MASK only); act [B,out]: WRITTEN by the forward, the layer's output after dropout (what the next
 *     layer reads; the backward reads it again), for l = L-1 the raw output before the epilogue.
 *   dropout (training mode; the caller passes VPN_FC_DROPOUT_OFF in eval mode): after layers 0..L-2, y = keep ? y / (1 - p)
 *     : 0.  VPN_FC_DROPOUT_PHILOX: keep = u >= p, u = (word0 >> 8) 2^-24 of Philox4x32-10 with key seed + *seed_dev
 *     (seed_dev NULL or a DEVICE uint64, as vpn_sample_fwd: a step counter, so that replays of a captured graph draw anew)
 *     and counter (o, b, l, g); never stored, the backward draws it again from the same arguments, so *seed_dev must
 *     not change between a forward and its backward.
 *   epilogue of the last layer: VPN_FC_NONE (the outputs are act of layer L-1); VPN_FC_TANH (G = 1): final [B,out] =
 *     tanh(raw); VPN_FC_VP_PACK (G = 3, outs 3K | 4K | 3K): final = the packed [B,K,10] rows that vpn_head_pack_fwd
 *     makes of the three raw outputs, same rule and same arguments.
 *   backward, VpnFcGrad: gout = dL/d(outputs): gout[g] [B,out] per group under VPN_FC_NONE, gout[0] = dL/dfinal otherwise;
 *     dw / db per slot, NULL = skipped (a frozen group costs nothing); dx[g] [B,in0[g]] per group, NULL = skipped (groups
 *     that share an input get separate gradients, the caller adds them).  workspace: vpn_fc_stack_workspace(G, B, the
 *     largest in / out of any layer) bytes, 16-byte aligned.
 *   L <= VPN_FC_MAX_LAYERS, G L <= VPN_FC_MAX_SLOTS, B (largest width) <= INT32_MAX / 4: VPN_E_TOOBIG beyond; null
 *   pointers and non-positive sizes: VPN_E_BADARG; all before any HIP call. */
#define VPN_FC_MAX_LAYERS 8
#define VPN_FC_MAX_SLOTS 24
#define VPN_FC_SLICE 32                /* weight rows per partial sum of the backward's dX */
#define VPN_FC_NONE 0
#define VPN_FC_TANH 1
#define VPN_FC_VP_PACK 2
#define VPN_FC_DROPOUT_OFF 0
#define VPN_FC_DROPOUT_MASK 1
#define VPN_FC_DROPOUT_PHILOX 2
typedef struct VpnFcStack {
    int32_t G, L, B, reserved;
    int32_t in0[VPN_FC_MAX_SLOTS];
    int32_t out[VPN_FC_MAX_SLOTS];
    const float* x[VPN_FC_MAX_SLOTS];
    const float* w[VPN_FC_MAX_SLOTS];
    const float* bias[VPN_FC_MAX_SLOTS];
    const uint8_t* keep[VPN_FC_MAX_SLOTS];
    float* act[VPN_FC_MAX_SLOTS];
} VpnFcStack;
typedef struct VpnFcGrad {
    const float* gout[VPN_FC_MAX_SLOTS];
    float* dw[VPN_FC_MAX_SLOTS];
    float* db[VPN_FC_MAX_SLOTS];
    float* dx[VPN_FC_MAX_SLOTS];
} VpnFcGrad;
size_t vpn_fc_stack_workspace(int G, int B, int max_width);
int vpn_fc_stack_fwd(VpnFcStack stack, int dropout, float p, uint64_t seed, const uint64_t* seed_dev, int epilogue, int K,
                     int is_sigmoid, float clamp_min, float clamp_max, float restrict0, float restrict1, float restrict2, float* final,
                     void* stream);
int vpn_fc_stack_bwd(VpnFcStack stack, VpnFcGrad grad, int dropout, float p, uint64_t seed, const uint64_t* seed_dev,
                     int epilogue, int K, int is_sigmoid, float clamp_min, float clamp_max, float restrict0, float restrict1, float restrict2,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- the optimiser stage (csrc/optim.hip; train.py:83-102 `Adam(params, lr, betas=(0.9, 0.99), weight_decay=W_DECAY)` and
 * train.py:264 `optimizer.step()` of the reference, the same two lines at train_sphere.py:92 / :134 and train_gcn.py:105 /
 * :138): Adam with torch's L2 weight decay over all parameters of one group in ONE plain launch, the step
 * counter and the bias-correction products on the device, gradient zeroing (optimizer.zero_grad(), train.py:262) folded into
 * the same pass.  No host synchronisation, nothing allocated, no second launch, no pow on the device; replayed from a
 * captured graph every replay is a fresh step.  Added without a change of VPN_ABI_VERSION.
 *   segments [S] VpnAdamSegment (DEVICE): one row per parameter that has a gradient: p, g, m, v [n] fp32 each; vec != 0:
 *     the four pointers are 16-byte aligned and the kernel uses 16-byte accesses (the caller decides, as below).
 *   chunks [C,2] int64 (DEVICE) = (segment, first element): one row per workgroup, which updates the elements [first,
 *     min(first + VPN_ADAM_CHUNK, n)) of that segment; first is a multiple of VPN_ADAM_CHUNK.  Both are clamped into the
 *     tables on the device (a bad row updates nothing and still arrives).
 *   state (DEVICE, VPN_ADAM_STATE_BYTES, 8-byte aligned) = {int64 step, double b1pow, double b2pow, uint32 arrivals, pad},
 *     {0, 1.0, 1.0, 0} before the first step.  Every workgroup reads it; the one that arrives last writes {step + 1,
 *     b1pow * beta1, b2pow * beta2, 0}.
 *   hyper (HOST, read before the call returns) = {lr, beta1, beta2, eps, weight_decay} as doubles (a pointer, because the
 *     binding passes no double by value); lr_dev: NULL, or a DEVICE float that the kernel reads INSTEAD of hyper[0]: a
 *     schedule written on the device, which a captured graph follows.
 *   arithmetic (the specification; tests/optim_ref.py restates it bit for bit): in double B1 = b1pow * beta1, B2 = b2pow *
 *     beta2, c1 = (float)(1 - beta1), c2 = (float)(1 - beta2), b2f = (float)beta2, wdf = (float)wd, epsf = (float)eps,
 *     bc2s = (float)sqrt(1 - B2), nss = (float)(-(lr / (1 - B1))); per element, fp32, every operation rounded by itself,
 *     IEEE sqrt and divide: g1 = wd != 0 ? g + wdf * p : g; m' = m + c1 * (g1 - m); v' = v * b2f + c2 * (g1 * g1);
 *     den = sqrt(v') / bc2s + epsf; p' = p + nss * (m' / den); zero_grads != 0: g = 0.  Non-finite values propagate.
 *   num_segments == 0: success, nothing is launched, the state does not advance.  Null pointers, num_chunks <= 0,
 *   misaligned tables or state, betas outside [0, 1), a negative or non-finite eps / weight_decay / lr: VPN_E_BADARG, before
 *   any HIP call. */
#define VPN_ADAM_CHUNK 4096            /* elements per workgroup: 256 lanes x 4 accesses of 16 bytes per array */
#define VPN_ADAM_STATE_BYTES 32
typedef struct VpnAdamSegment {
    float* p;
    float* g;
    float* m;
    float* v;
    long long n;
    long long vec;
} VpnAdamSegment;
/* bytes of a table for `segments` rows and `elements` parameters in all: segments * sizeof(VpnAdamSegment) + 16 * (elements /
 * VPN_ADAM_CHUNK + segments), the most chunk rows they can have; 0 for a negative argument */
size_t vpn_adam_table_bytes(int segments, long long elements);
int vpn_adam_step(const VpnAdamSegment* segments, int num_segments, const long long* chunks, int num_chunks, void* state,
                  const double* hyper, const float* lr_dev, int zero_grads, void* stream);

/* ---- the trunk's norm / add / ReLU ring (csrc/trunknorm.hip; the torchvision ResNet-18 of vpnet_one_resnet.py:21,
 * vpnet_two_resnet.py:21-22 and sdnet.py:13 of the reference): batch norm over (B, H, W) per channel, then
 * `+ residual`, then ReLU, as ONE op forward and backward.  All tensors DEVICE fp32, NCHW contiguous, 4-byte aligned; the
 * kernels use 16-byte accesses when H * W is a multiple of 4 and every [B,C,H,W] pointer of the call is 16-byte aligned,
 * element accesses otherwise (decided per call, no error).  N = B * H * W elements per channel.  No host synchronisation,
 * nothing allocated, no atomics: bit-equal from run to run, capturable.  Added without a change of VPN_ABI_VERSION
 * (DESIGN.md 4.10).
 *   N <= VPN_BN_ONE_PASS_MAX: one launch per call, no workspace (workspace may be NULL).  Larger N: two launches over
 *   slices of VPN_BN_SLICE elements and a workspace of vpn_bn_act_workspace(B, C, H, W) bytes (4-byte aligned,
 *   uninitialised: C * ceil(N / VPN_BN_SLICE) * 2 floats), 0 bytes in the one-launch case.
 * vpn_bn_act_fwd, training != 0: mean, biased var, invstd = 1 / sqrt(var + eps) per channel (exact-mean second pass, Chan's
 *   merge of the slices: no E[x^2] - E[x]^2); y = (x - mean) * invstd * weight + bias, + residual when residual != NULL,
 *   max(., 0) when relu != 0; save_mean [C], save_invstd [C] written; running_mean / running_var [C] (each may be NULL)
 *   updated in place as (1 - momentum) * r + momentum * stat, the variance unbiased by N / (N - 1); num_batches_tracked
 *   (int64, may be NULL) incremented by one.  training == 0: the running statistics are read, one elementwise launch,
 *   save_mean / save_invstd / num_batches_tracked / workspace are not touched (may be NULL).
 *   weight, bias: [C] or NULL (1 and 0).  y must not alias x or residual.
 * vpn_bn_act_bwd: g = dy * [y > 0] when relu != 0 (y: the forward's output; NULL allowed when relu == 0), else g = dy.
 *   training != 0: stat_mean / stat_var = save_mean / save_invstd of the forward; d_bias = sum g, d_weight = sum g * xhat,
 *   dx = weight * invstd * (g - d_bias / N - xhat * d_weight / N).  training == 0: stat_mean / stat_var = running_mean /
 *   running_var, dx = g * weight / sqrt(running_var + eps), the two sums only when d_weight or d_bias is wanted.
 *   d_residual = g.  dx, d_residual, d_weight, d_bias: each may be NULL and is then neither computed nor written (dx still
 *   uses both sums); all four NULL: nothing is launched.  The workspace is needed when N > VPN_BN_ONE_PASS_MAX unless
 *   training == 0 and d_residual, d_weight and d_bias are all NULL.
 * Non-positive sizes, a required pointer that is NULL, N == 1 in training, eps < 0, momentum outside [0, 1], a workspace
 * that is missing, too small or misaligned: VPN_E_BADARG.  N >= 2^31 or more than 65535 slices: VPN_E_TOOBIG.  Both before
 * any HIP call. */
#define VPN_BN_ONE_PASS_MAX 8192       /* floats of a channel held in LDS: 32 KB forward, 64 KB backward (g and xhat) */
#define VPN_BN_SLICE 2048              /* elements per workgroup in the two-launch regime: 256 lanes x 8 */
size_t vpn_bn_act_workspace(int B, int C, int H, int W);
int vpn_bn_act_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* running_mean,
                   float* running_var, long long* num_batches_tracked, int B, int C, int H, int W, int training, float momentum,
                   float eps, int relu, float* y, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                   void* stream);
int vpn_bn_act_bwd(const float* dy, const float* x, const float* y, const float* weight, const float* stat_mean,
                   const float* stat_var, int B, int C, int H, int W, int training, float eps, int relu, float* dx,
                   float* d_residual, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trunk's stem: batch norm, ReLU and MaxPool2d(3, 2, 1) as ONE op, forward and backward (the tp_ kernels of
 * csrc/trunknorm.hip; `maxpool(relu(bn1(conv1(x))))` of the torchvision ResNet-18).  The pool is fixed:
 * kernel 3, stride 2, padding 1, dilation 1, the only pool of the reference's networks.  x, dx: [B,C,H,W]; p, dp: [B,C,PH,PW]
 * with PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1; idx: [B,C,PH,PW] uint8.  All DEVICE, fp32 but idx, contiguous, 4-byte
 * aligned (idx: any).  Window (ph, pw) covers rows 2 ph - 1 .. 2 ph + 1 and columns 2 pw - 1 .. 2 pw + 1; taps outside the map
 * take no part.  y = max((x - mean) * invstd * weight + bias, 0) per tap with the roundings of vpn_bn_act_fwd, p = the
 * maximum of the window's taps, idx = the tap number r * 3 + s (0 .. 8) of the winner: taps are scanned r then s ascending
 * and a tap replaces the best so far only if it is greater or is NaN (ATen's rule: the first maximum wins).  The full-size
 * y is never written.  The windows and the backward access x and dx 16 bytes at a time when W is a multiple of 4 and x (and
 * dx) is 16-byte aligned, the statistics when H * W is and x is aligned; element accesses otherwise (decided per call, no
 * error).  No host synchronisation, nothing allocated, no atomics: bit-equal from run to run, capturable.  Added without a
 * change of VPN_ABI_VERSION.
 * vpn_bn_pool_workspace: C * ceil(N / VPN_BN_SLICE) * 2 floats in bytes, N = B * H * W; 0 for sizes the entries refuse.
 * vpn_bn_pool_fwd, training != 0: the statistics of vpn_bn_act_fwd by the same code: save_mean, save_invstd [C] written,
 *   running_mean / running_var (each may be NULL) and num_batches_tracked (int64, may be NULL) updated, all bit-equal to
 *   what vpn_bn_act_fwd writes for the same x.  N <= VPN_BN_ONE_PASS_MAX: ONE launch (the channel's slab stays in LDS between
 *   the statistics and the windows), no workspace (may be NULL).  Larger N: TWO launches, the statistics launch of
 *   vpn_bn_act_fwd over slices of VPN_BN_SLICE elements into the workspace (4-byte aligned, uninitialised), then one over
 *   slices of VPN_BN_POOL_SLICE pooled outputs that merges them and writes p and idx.  training == 0: ONE launch on the
 *   running statistics; save_mean / save_invstd / num_batches_tracked / workspace are not touched (may be NULL).
 *   weight, bias: [C] or NULL (1 and 0).  Written: p, idx and the statistics named above, nothing else.
 * vpn_bn_pool_bwd: the upstream gradient of pixel (h, w) is g = sum dp[ph,pw] * [p[ph,pw] > 0] over the at most four windows
 *   that contain the pixel and whose idx names it, ph then pw ascending; then the arithmetic of vpn_bn_act_bwd: d_bias =
 *   sum g, d_weight = sum g * xhat, dx = weight * invstd * (g - d_bias / N - xhat * d_weight / N); training == 0: stat_mean /
 *   stat_var = running_mean / running_var and dx = g * weight / sqrt(running_var + eps).  Reads dp, p, idx, x and the two
 *   statistics.  At most TWO launches for every N: the two sums per slice of VPN_BN_SLICE elements into the workspace, then
 *   their merge (the order of vpn_bn_act_bwd) and dx; ONE when training == 0 and d_weight and d_bias are NULL (no workspace
 *   needed then).  dx, d_weight, d_bias: each may be NULL and is then neither computed nor written; all NULL: nothing is
 *   launched.
 * Non-positive sizes, a required pointer that is NULL, N == 1 in training, eps < 0, momentum outside [0, 1], a needed
 * workspace that is missing, too small or misaligned: VPN_E_BADARG.  N >= 2^31, more than 65535 slices of either kind:
 * VPN_E_TOOBIG.  Both before any HIP call. */
#define VPN_BN_POOL_SLICE 512          /* pooled outputs per workgroup of the pooling launch: 256 lanes x 2 */
size_t vpn_bn_pool_workspace(int B, int C, int H, int W);
int vpn_bn_pool_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                    long long* num_batches_tracked, int B, int C, int H, int W, int training, float momentum, float eps,
                    float* p, unsigned char* idx, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                    void* stream);
int vpn_bn_pool_bwd(const float* dp, const float* x, const float* p, const unsigned char* idx, const float* weight,
                    const float* stat_mean, const float* stat_var, int B, int C, int H, int W, int training, float eps,
                    float* dx, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trunk's tail: the last norm / add / ReLU site and the global average pool as ONE op, forward and backward (the
 * tt_ kernels of csrc/trunknorm.hip; `avgpool(layer4(.))` of the torchvision ResNet-18).  x, residual, y, dy,
 * dx, d_residual: [B,C,H,W]; m, dm: [B,C].  All DEVICE fp32, contiguous, 4-byte aligned; 16-byte accesses under the rule of
 * vpn_bn_act_* (m and dm are always accessed by element).  A row is the H * W elements of one (b, c).
 *   m[b,c] = (sum over hw of y[b,c,hw]) / (float)(H * W): an fp32 sum in one fixed order, then ONE fp32 division.  The order:
 *   where the rows a workgroup owns fit LDS (every case but rows longer than VPN_BN_SLICE outside the one-launch regime), a
 *   group of G lanes, G the smallest power of two >= min(H * W, 64), owns a row, lane j adds the elements j, j + G, ... in
 *   order, then the group's butterfly; a longer row is owned by one workgroup, a work-item adds its elements in order, then
 *   the wave's butterfly, then the waves in order.
 *   The upstream gradient of an element is dy[b,c,hw] + dm[b,c] / (float)(H * W): one IEEE fp32 division per row, then one
 *   fp32 addition.
 * No host synchronisation, nothing allocated, no atomics: bit-equal from run to run, capturable.  Added without a change of
 * VPN_ABI_VERSION.
 * vpn_bn_tail_workspace: the rule of vpn_bn_act_workspace: C * ceil(N / VPN_BN_SLICE) * 2 floats in bytes when N = B * H * W >
 *   VPN_BN_ONE_PASS_MAX, else 0; 0 for sizes the entries refuse.
 * vpn_bn_tail_fwd: y, save_mean, save_invstd, the running statistics and num_batches_tracked are what vpn_bn_act_fwd writes
 *   for the same arguments, bit for bit; m is written in addition.  residual and relu are optional as there.  training != 0
 *   and N <= VPN_BN_ONE_PASS_MAX: ONE launch (the rows are summed from the channel's slab in LDS), no workspace.  Larger N:
 *   TWO launches, the statistics launch of vpn_bn_act_fwd, then an apply launch on a grid (C, ceil(B / R)) whose workgroups
 *   own R = max(VPN_BN_SLICE / (H * W), 1) whole batch rows of a channel.  training == 0: ONE launch, the apply launch on the
 *   running statistics.
 * vpn_bn_tail_bwd: vpn_bn_act_bwd on the upstream gradient above: g, the two sums, dx, d_residual, d_weight and d_bias
 *   follow it exactly, with its launch counts and its workspace rule.  dy NULL: no gradient reaches the map, the upstream
 *   gradient is dm[b,c] / (H * W) and dy is not read.  dm NULL: the call equals vpn_bn_act_bwd bit for bit.  Both NULL:
 *   VPN_E_BADARG.  dx, d_residual, d_weight, d_bias all NULL: nothing is launched.
 * The rules of vpn_bn_act_fwd / _bwd, and m == NULL: VPN_E_BADARG.  N >= 2^31, more than 65535 slices, or an apply grid with
 * ceil(B / R) > 65535: VPN_E_TOOBIG.  Both before any HIP call. */
size_t vpn_bn_tail_workspace(int B, int C, int H, int W);
int vpn_bn_tail_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* running_mean,
                    float* running_var, long long* num_batches_tracked, int B, int C, int H, int W, int training, float momentum,
                    float eps, int relu, float* y, float* m, float* save_mean, float* save_invstd, void* workspace,
                    size_t workspace_bytes, void* stream);
int vpn_bn_tail_bwd(const float* dy, const float* dm, const float* x, const float* y, const float* weight,
                    const float* stat_mean, const float* stat_var, int B, int C, int H, int W, int training, float eps, int relu,
                    float* dx, float* d_residual, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- the trunk's 3x3 convolutions (csrc/trunkconv.hip): kernel 3x3, stride 1, padding 1, dilation 1,
 * groups 1, no bias, as an implicit GEMM on the f32-input MFMA: exact fp32 products, one fixed summation order.  All tensors
 * DEVICE fp32, contiguous, 4-byte aligned: x [B,C_in,H,W], w [C_out,C_in,3,3], y and dy [B,C_out,H,W], dx as x, dw as w.  Any
 * positive sizes; padding and the tails of every tile are masked loads.  No host synchronisation, nothing allocated, no
 * atomics: bit-equal from run to run, capturable.  Added without a change of VPN_ABI_VERSION.
 *   A product is a GEMM of M x N outputs over K: forward M = C_out, N = B H W, K = 9 C_in; data gradient M = C_in,
 *   N = B H W, K = 9 C_out; weight gradient M = C_out, N = 9 C_in, K = B H W.  A workgroup owns VPN_CONV_TILE x VPN_CONV_TILE
 *   outputs and walks K in chunks of VPN_CONV_TILE_K.  With tiles = ceil(M / TILE) ceil(N / TILE) < VPN_CONV_SPLIT_TARGET the
 *   chunks are split over S = min(ceil(VPN_CONV_SPLIT_TARGET / tiles), VPN_CONV_MAX_SPLIT, chunks) slices (vpn_conv3x3_splits
 *   returns S, 1 when unsplit, or a negative VPN_E_* code), the partial results go to `workspace` ([S][outputs] floats, 16-byte
 *   aligned, uninitialised) and a second launch adds them in the order 0 .. S - 1.
 * vpn_conv3x3_workspace: the bytes a call needs for the products in `products` (VPN_CONV_FWD | VPN_CONV_DX | VPN_CONV_DW; a
 *   backward call uses one workspace for both of its products in turn: the larger of the two); 0 when none is needed (or for
 *   sizes the entries reject).
 * vpn_conv3x3_fwd replaces the forward of nn.Conv2d inside torchvision's BasicBlock, reached through the reference's
 *   vpnet_one_resnet.py:45-57:  y[b,co,h,w] = sum_{ci,r,s} x[b,ci,h+r-1,w+s-1] w[co,ci,r,s].
 * vpn_conv3x3_bwd replaces that module's backward (ATen's convolution_backward under the same lines):
 *   dx[b,ci,h,w] = sum_{co,r,s} dy[b,co,h+1-r,w+1-s] w[co,ci,r,s] (the forward's kernel reading w with the channel strides
 *   swapped and the taps mirrored: no transposed copy), dw[co,ci,r,s] = sum_{b,h,w} dy[b,co,h,w] x[b,ci,h+r-1,w+s-1].  dx or dw
 *   may be NULL: that product is neither computed nor stored; both NULL: nothing is launched.
 * dy / x / w / y NULL or a non-positive size: VPN_E_BADARG; a workspace that is needed and missing, too small or not 16-byte
 * aligned: VPN_E_BADARG; a tensor of 2^31 elements or more, or more than 65535 tiles along M: VPN_E_TOOBIG.  All before any
 * HIP call. */
#define VPN_CONV_TILE 64               /* outputs along M and along N of one workgroup: 2 x 2 waves of 32 x 32 MFMA tiles */
#define VPN_CONV_TILE_K 16             /* reduction elements per LDS chunk: slices are whole chunks */
#define VPN_CONV_SPLIT_TARGET 256      /* fewer tiles than this (the CUs of an MI355X): split K to reach it */
#define VPN_CONV_MAX_SPLIT 32          /* most slices of one product */
#define VPN_CONV_FWD 1                 /* the products, as bits of vpn_conv3x3_workspace's `products` */
#define VPN_CONV_DX 2
#define VPN_CONV_DW 4
size_t vpn_conv3x3_workspace(int B, int C_in, int C_out, int H, int W, int products);
int vpn_conv3x3_splits(int B, int C_in, int C_out, int H, int W, int product);
int vpn_conv3x3_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream);
int vpn_conv3x3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trunk's strided convolutions (csrc/trunkstride.hip): square kernel R in {1, 3, 7}, stride >= 1,
 * padding >= 0, dilation 1, groups 1, no bias, by the scheme and with the VPN_CONV_* constants of vpn_conv3x3_* above: exact
 * fp32 products, one fixed summation order.  OH = (H + 2 pad - R) / stride + 1 (floor), OW likewise.  All tensors DEVICE fp32,
 * contiguous, 4-byte aligned: x [B,C_in,H,W], w [C_out,C_in,R,R], y and dy [B,C_out,OH,OW], dx as x, dw as w.  Padding, stride
 * gaps and the tails of every tile are masked loads.  No host synchronisation, nothing allocated, no atomics: bit-equal from
 * run to run, capturable.  Added without a change of VPN_ABI_VERSION.
 *   A product is a GEMM of M x N outputs over K: forward M = C_out, N = B OH OW, K = R R C_in; data gradient M = C_in,
 *   N = B H W, K = R R C_out; weight gradient M = C_out, N = R R C_in, K = B OH OW.  Tiles, slices and the workspace follow the
 *   rule stated at vpn_conv3x3_*: vpn_conv2d_splits returns S (1 when unsplit, or a negative VPN_E_* code),
 *   vpn_conv2d_workspace the bytes for the products in `products` (the larger of a backward call's two; 0 when none is needed
 *   or for arguments the entries reject).  With (R, stride, pad) = (3, 1, 1) both equal vpn_conv3x3_splits / _workspace and the
 *   results equal vpn_conv3x3_fwd / _bwd bit for bit.
 * vpn_conv2d_fwd replaces the forward of nn.Conv2d reached through the reference's vpnet_one_resnet.py:45-57 (the 7x7 stem,
 *   the stride-2 3x3 and the 1x1 downsample convolutions of torchvision's resnet18):
 *   y[b,co,oh,ow] = sum_{ci,r,s} x[b,ci,oh stride+r-pad,ow stride+s-pad] w[co,ci,r,s].
 * vpn_conv2d_bwd replaces that module's backward (ATen's convolution_backward under the same lines):
 *   dx[b,ci,ih,iw] = sum_{co,r,s} dy[b,co,(ih+pad-r)/stride,(iw+pad-s)/stride] w[co,ci,r,s] over the taps whose two quotients
 *   are exact and in range (an input pixel that no output reads gets dx = 0, written by the call: dx need not be zeroed),
 *   dw[co,ci,r,s] = sum_{b,oh,ow} dy[b,co,oh,ow] x[b,ci,oh stride+r-pad,ow stride+s-pad].  dx or dw may be NULL: that product is
 *   neither computed nor stored; both NULL: nothing is launched.
 * dy / x / w / y NULL, a non-positive size, R not 1, 3 or 7, stride < 1, pad < 0, H + 2 pad < R or W + 2 pad < R:
 * VPN_E_BADARG; a workspace that is needed and missing, too small or not 16-byte aligned: VPN_E_BADARG; x, y or w of 2^31
 * elements or more, H + 2 pad or W + 2 pad of 2^31 or more, or more than 65535 tiles along M: VPN_E_TOOBIG.  All before any HIP
 * call. */
size_t vpn_conv2d_workspace(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int products);
int vpn_conv2d_splits(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int product);
int vpn_conv2d_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, int R, int stride, int pad,
                   void* workspace, size_t workspace_bytes, void* stream);
int vpn_conv2d_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H, int W,
                   int R, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trunk's convolutions for eval-mode inference (csrc/trunkfold.hip): vpn_conv2d_fwd's product with
 * an epilogue, forward only:  y = act(conv(x, w) + bias[c_out] + residual), act the ReLU when relu = 1, the identity when 0.
 * It replaces nn.Conv2d + nn.BatchNorm2d (eval) + add + ReLU reached through the reference's vpnet_one_resnet.py:45-57 once the
 * norm's fixed scale has been multiplied into w and its shift is `bias` (a fold the caller makes once; all 20 convolution sites
 * of the ResNet-18 trunk when nothing is trained: train_gcn.py:100-125, test.py, test_gcn.py).
 * x, w, y as vpn_conv2d_fwd; bias DEVICE fp32 [C_out] or NULL; residual DEVICE fp32 of y's shape, contiguous, or NULL; it may
 * not overlap y.  Per element, in this order: v = conv + bias[c_out]; v += residual; v = v < 0 ? 0 : v (a NaN stays a NaN).
 * With bias and residual NULL and relu 0 the result equals vpn_conv2d_fwd's bit for bit.
 * The slices and the workspace are vpn_conv2d_splits(..., VPN_CONV_FWD) and vpn_conv2d_workspace(..., VPN_CONV_FWD): an unsplit
 * product applies the epilogue at its store (one launch); a split one writes raw partials and the launch that adds them in the
 * order 0 .. S - 1 applies it (two launches).  No host synchronisation, nothing allocated, no atomics: bit-equal from run to
 * run, capturable.  Added without a change of VPN_ABI_VERSION.
 * Every rejection of vpn_conv2d_fwd, with its code; relu not 0 or 1: VPN_E_BADARG.  All before any HIP call. */
int vpn_conv2d_bias_act_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int C_in,
                            int C_out, int H, int W, int R, int stride, int pad, int relu, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---- mesh regularisers (csrc/meshreg.hip): the edge-length, uniform-Laplacian (squared) and
 * normal-consistency terms of Pixel2Mesh (Wang et al., ECCV 2018) on verts DEVICE fp32 [B,V,3] over ONE face topology shared
 * by the batch.  out DEVICE fp32 [3] = (edge, lap, normal):
 *   edge    mean over (b, e) of (|v_a - v_b| - edge_target)^2, as |v_a - v_b|^2 without a root when edge_target == 0; with
 *           edge_target > 0 an edge of length exactly 0 has gradient 0.
 *   lap     mean over (b, i), all V vertices, of |delta_i|^2, delta_i = (1 / deg_i) sum_{j in N(i)} v_j - v_i, 0 when deg_i = 0.
 *   normal  mean over (b, pair) of 1 - s n_f.n_g / (max(|n_f|, 1e-8) max(|n_g|, 1e-8)), n_f = (v1 - v0) x (v2 - v0); a
 *           clamped norm is a constant in the gradient.  0 when P = 0; edge and lap are 0 when E = 0.
 * The tables are DEVICE int32, built on the host (ops.mesh_topology): faces [F,3]; edges [E,2], unique, a < b; nbr_ptr [V+1]
 * / nbr [2E], the neighbours of a vertex in CSR form; adj [F,3], for edge j = (corner j, corner j + 1) of a face the adjacent
 * face g of the pair across it as 2 g + (s < 0), or -1 (every edge with exactly two incident faces is one pair; a face
 * with a repeated index is incident to nothing); vf_ptr [V+1] / vf, per vertex the (face, corner) it is of faces with a pair,
 * as 4 f + corner.  P: the number of pairs.  Index values are NOT checked on the device.
 * terms: bits VPN_MESHREG_EDGE | _LAP | _NORMAL; a term whose bit is absent is not computed, its value is 0 and it adds
 *   nothing to the gradient, whatever its upstream gradient.
 * vpn_meshreg_fwd: two launches (per-workgroup sums over 256-item chunks, then their sum in a fixed order); workspace:
 *   vpn_meshreg_workspace(B, V, E, F) bytes (0: rejected shapes).  delta [B,V,3] and normals [B,F,3] (either may be NULL: not
 *   written) are what the backward reads: delta under the LAP bit, normals under the NORMAL bit.
 * vpn_meshreg_bwd: one launch, a gather per vertex: dverts [B,V,3] = sum_k grad[k] d out[k] / d verts with grad DEVICE fp32
 *   [3]; delta (LAP) and normals (NORMAL, when P > 0) as the forward wrote them with the same terms and edge_target.
 * No host synchronisation, nothing allocated, no atomics: bit-equal from run to run, capturable.  Any vertex degree.
 * B <= 65535, V, E, F <= VPN_MESHREG_MAX_ITEMS: VPN_E_TOOBIG beyond.  Null pointers (edges and nbr may be NULL when E = 0, vf
 * when P = 0), B, V or F < 1, E or P < 0, terms outside 0..7, an edge_target that is negative or not finite: VPN_E_BADARG.
 * All before any HIP call.  Added without a change of VPN_ABI_VERSION. */
#define VPN_MESHREG_EDGE 1
#define VPN_MESHREG_LAP 2
#define VPN_MESHREG_NORMAL 4
#define VPN_MESHREG_CHUNK 256          /* items (edges, vertices, faces) per workgroup and per partial sum of the forward */
#define VPN_MESHREG_MAX_ITEMS 16777216
size_t vpn_meshreg_workspace(int B, int V, int E, int F);
int vpn_meshreg_fwd(const float* verts, const int32_t* faces, const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr,
                    const int32_t* adj, int B, int V, int E, int F, int P, float edge_target, int terms, void* workspace,
                    float* delta, float* normals, float* out, void* stream);
int vpn_meshreg_bwd(const float* grad, const float* verts, const float* delta, const float* normals, const int32_t* faces,
                    const int32_t* nbr_ptr, const int32_t* nbr, const int32_t* vf_ptr, const int32_t* vf, const int32_t* adj,
                    int B, int V, int E, int F, int P, float edge_target, int terms, float* dverts, void* stream);

/* ---- point-to-surface distance (csrc/pointmesh.hip): the squared Euclidean distance between points DEVICE
 * fp32 [B,P,3] and the closed triangles of verts DEVICE fp32 [B,V,3] over ONE face list faces DEVICE int32 [F,3] for the
 * batch, both ways (the point_mesh_face_distance of PyTorch3D):
 *   d(p, T)   min over the simplex w of |p - (w0 v0 + w1 v1 + w2 v2)|^2, formed from p - c, c the closest point.  A
 *             triangle without area is the segment or the point it degenerates to and is still a face.
 *   dist_p [B,P], face_of_point [B,P] int32   min over the faces and the lowest face that gives it;
 *   dist_f [B,F], point_of_face [B,F] int32   min over the points and the lowest point that gives it;
 *   out [2] = (mean of dist_p over (b, i), mean of dist_f over (b, f)).
 * "Lowest" is by strict < from (inf, index 0) among the values computed: every index written lies in [0, F) / [0, P)
 * whatever the coordinates hold, NaN and inf included.  Index values of faces are NOT checked on the device.
 * vpn_pointmesh_fwd: at most four launches (face records, the pair scan over (256-point tile, face slice, sample), the merge
 *   of the partial minima with the chunk sums, the two means).  dist_p, face_of_point, dist_f, point_of_face and out may
 *   each be NULL: not written.  workspace: at least vpn_pointmesh_workspace(B, P, V, F) bytes (0: rejected shapes).
 * vpn_pointmesh_bwd: at most three launches, no scatter: per face the points that chose it (a scan of face_of_point), per
 *   point the faces that chose it (a scan of point_of_face), a gather per vertex over vf_ptr [V+1] / vf [3F], DEVICE int32,
 *   per vertex 4 f + corner of EVERY face it is a corner of, ascending.  grad DEVICE fp32 [2]; with c and w of the saved
 *   index, d d / d p = 2 (p - c), d d / d v_k = -2 w_k (p - c).  dpoints [B,P,3] and dverts [B,V,3] may each be NULL: not
 *   computed (vf_ptr, vf and workspace are needed for dverts only).  The same workspace size serves.
 * No host synchronisation, nothing allocated, no atomics: bit-equal from run to run, capturable.
 * Null pointers, B, P, V or F < 1, a workspace shorter than needed: VPN_E_BADARG.  B > 65535 or P, V or F >
 * VPN_POINTMESH_MAX_ITEMS: VPN_E_TOOBIG.  All before any HIP call.  Added without a change of VPN_ABI_VERSION. */
#define VPN_POINTMESH_TILE 256           /* points per workgroup of the pair scan */
#define VPN_POINTMESH_MIN_SLICE 128      /* a face slice of the pair scan has at least this many faces (but for the last) */
#define VPN_POINTMESH_MAX_SLICES 64
#define VPN_POINTMESH_MAX_ITEMS 1048576
size_t vpn_pointmesh_workspace(int B, int P, int V, int F);
int vpn_pointmesh_fwd(const float* points, const float* verts, const int32_t* faces, int B, int P, int V, int F, void* workspace,
                      size_t workspace_bytes, float* dist_p, int32_t* face_of_point, float* dist_f, int32_t* point_of_face,
                      float* out, void* stream);
int vpn_pointmesh_bwd(const float* grad, const float* points, const float* verts, const int32_t* faces,
                      const int32_t* face_of_point, const int32_t* point_of_face, const int32_t* vf_ptr, const int32_t* vf, int B,
                      int P, int V, int F, void* workspace, size_t workspace_bytes, float* dpoints, float* dverts, void* stream);

/* ---- surface evaluation (csrc/surfeval.hip): the metrics of single-view reconstruction on points sampled
 * from the predicted SURFACE, per sample, and the per-class bookkeeping of an evaluation epoch on the device.
 * vpn_face_normals_at: the unit normal of the face every sampled point lies on, one launch, DEVICE pointers.
 *   batched layout (vert_offset and face_offset NULL): verts fp32 [B,P,3], ONE faces int32 [F,3] for the batch, fidx int32
 *     [B,n] in [0,F) (what vpn_mesh_sample_fwd returns); sets is not used (pass 1).
 *   ragged layout (both offsets given; the ground truth of a packed mesh batch): verts [P,3] with P = sumP, faces [F,3] with
 *     F = sumF and MESH-LOCAL vertex indices, vert_offset / face_offset int32 [S+1], fidx [B,n] mesh-local with B = S sets
 *     (what vpn_ragged_sample returns); sample b belongs to mesh b / sets.
 *   xforms fp32 [B,3,4] or NULL: affine rows (R | t); the three corners are mapped first (x' = m0 x + m1 y + m2 z + m3, summed
 *     left to right) and the normal is taken from the mapped corners, which is right for any affine map without an
 *     inverse-transpose; a map of negative determinant flips the sign.
 *   normals fp32 [B,n,3]: e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2, n = c / sqrtf(c.c), every operation rounded by itself;
 *     (0,0,0) where c.c is 0 or not finite, where the face index lies outside its range or a vertex index outside its mesh
 *     (nothing is read out of range).
 * vpn_surfeval_accumulate: two launches on `stream` (one workgroup per sample, then ONE workgroup for the bookkeeping; no
 *   ticket, no atomics).  dist1 [B,N] / idx1 [B,N] (prediction -> ground truth) and dist2 [B,M] / idx2 [B,M]: the distances
 *   and int32 indices as vpn_chamfer_fwd_ws writes them, that is EUCLIDEAN, NOT squared, distances d (the reference's Chamfer
 *   takes the root); below, d^2 is the product formed in fp64, where it is exact; n_pred [B,N,3] and n_gt [B,M,3]: unit normals, both or
 *   neither; thr2 [T]: SQUARED distance thresholds, fp32 on the device; class_index [B] int32.  Writes per_sample [B,W] fp32,
 *   W = 6 + 3 T:
 *     [0] acc2 = mean_i dist1^2    [1] comp2 = mean_j dist2^2
 *     [2] acc1 = mean_i dist1      [3] comp1 = mean_j dist2
 *     [4] nc1 = mean_i |n_pred[i] . n_gt[idx1[i]]|    [5] nc2 = mean_j |n_gt[j] . n_pred[idx2[j]]|   (0 without normals; the
 *         dot product is the fp64 sum of fp64 products; a neighbour index outside its range is clamped into it)
 *     [6, 6+T) precision_t = #{i : dist1[i]^2 < thr2[t]} / N    [6+T, 6+2T) recall_t = #{j : dist2[j]^2 < thr2[t]} / M
 *         (the exact fp64 square against the fp32 threshold: no rounding decides a count)
 *     [6+2T, 6+3T) fscore_t = 2 P R / (P + R), 0 when P + R = 0
 *   Counts are integers (a NaN distance is a miss); P, R and F are formed in fp64 from them and rounded once.  Every
 *   floating sum is taken in fp64 in ONE order (lane t of 256 owns elements t, t + 256, ...; xor tree over the wave; the
 *   four waves (0 + 1) + (2 + 3)), divided and rounded to fp32 once: bit-equal from run to run.
 *   state: vpn_surfeval_state_size(C, T) bytes (0: rejected sizes), 8-byte aligned, ZEROED BY THE CALLER before the first
 *   batch of an epoch: (1 + C) W doubles -- total[W], then class_sum[C][W] -- followed by 3 + C int64 -- n_samples,
 *   n_batches, n_invalid, class_n[C].  In sample order b = 0 .. B-1 and in fp64 (Python's `+= float(x)`): total[k] +=
 *   per_sample[b,k]; class_sum[c][k] += per_sample[b,k] and class_n[c] += 1 for c = class_index[b]; a class index outside
 *   [0, C) enters the totals, no class, and n_invalid.  Totals are SAMPLE-weighted: divide by n_samples (vpn_eval_accumulate
 *   adds batch means instead, which is the reference's rule for its own two metrics).  Two states are merged by adding them
 *   field by field.  Launches on one state must be ordered (one stream).
 * Nothing is allocated, no host synchronisation, capturable.  A null pointer (xforms, n_pred and n_gt may be NULL), a
 * non-positive size, one offset table or one normal tensor without the other, B no multiple of sets in the ragged layout, a
 * misaligned state: VPN_E_BADARG.  T > VPN_SURFEVAL_MAX_THRESHOLDS, B > 65535, N, M, n, P, F or C above
 * VPN_SURFEVAL_MAX_ITEMS: VPN_E_TOOBIG.  All before any HIP call.  Added without a change of VPN_ABI_VERSION (DESIGN.md
 * 4.10). */
#define VPN_SURFEVAL_MAX_THRESHOLDS 8
#define VPN_SURFEVAL_MAX_ITEMS 16777216
size_t vpn_surfeval_state_size(int num_classes, int T);
int vpn_face_normals_at(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                        const int32_t* fidx, const float* xforms, int B, int n, int P, int F, int sets, float* normals,
                        void* stream);
int vpn_surfeval_accumulate(const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2, const float* n_pred,
                            const float* n_gt, const float* thr2, const int32_t* class_index, int B, int N, int M, int T,
                            int num_classes, void* state, float* per_sample, void* stream);

/* ---- volumetric evaluation (csrc/occupancy.hip): occupancy of a primitive assembly and of a triangle mesh at
 * query points, and the intersection over union of two occupancies per sample with the per-class bookkeeping of an epoch on
 * the device.  DEVICE pointers.  queries fp32: [Q,3] shared by the batch (shared_queries != 0) or [B,Q,3] (0); both are read by
 * the same code (a sample stride of 0), so repeating a shared set B times gives the same bits.
 * vpn_occupancy_prims: one launch.  params fp32 [B,K,VPN_PARAM_STRIDE], kinds int32 [K].  Per primitive x~ = R^T (x - t) / v, R
 *   from q as the sampler and the raster form it, v the half-extents; m = x~.x~ (VPN_SPHERE) or max |x~_i| (any other kind: a
 *   cuboid); inside iff m <= 1, every operation in fp32 and rounded by itself; a NaN is outside.  occ uint8 [B,Q] = 0 / 1, the
 *   OR over k; owner int32 [B,Q] = the lowest k that holds the point, -1 for none.  occ or owner may be NULL: not written.
 * vpn_winding_number: three launches (face records, the scan over (256-query tile, face slice, sample), the merge).  The
 *   generalized winding number w = sum_f 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi with a, b, c the
 *   corners of face f minus x (Van Oosterom and Strackee), the terms in fp32 and exactly 0 where the numerator is 0 (a face of no
 *   area, a query on the face's plane or on a vertex), the sum in fp64 in ONE order (ascending faces within a slice, ascending
 *   slices), divided by 4 pi in fp64 and rounded to fp32 once.  A face with a vertex index outside its mesh adds nothing and reads
 *   nothing out of range, nor does a face whose edge cross product (v1 - v0) x (v2 - v0) is (0,0,0) in fp32; a live face with a corner that is not finite, or a query that is not finite, makes w NaN.
 *   batched layout (vert_offset and face_offset NULL): verts fp32 [B,P,3], ONE faces int32 [F,3]; max_faces is not used.
 *   ragged layout (both given; a packed mesh batch): verts [P,3] with P = sumP, faces [F,3] with F = sumF and MESH-LOCAL vertex
 *     indices, vert_offset / face_offset int32 [B+1]; sample b is mesh b.  max_faces: the largest face count of a mesh, known
 *     on the host (1 .. F); it sizes the grid only: a mesh with more faces is still summed whole, by its last slice.  An
 *     offset entry that does not describe the packed arrays names no face.
 *   xforms fp32 [B,3,4] or NULL: affine rows applied to the corners first, as vpn_face_normals_at does; a map of negative
 *     determinant negates w.
 *   w fp32 [B,Q] and occ uint8 [B,Q] = (w > 0.5, on the rounded value; NaN is outside) may each be NULL (not both).
 *   workspace: at least vpn_winding_workspace(B, Q, F, ragged, max_faces) bytes (0: rejected shapes), 16-byte aligned.
 *   vpn_winding_plan returns the number of face slices (or a negative code) and writes the faces per slice: a function of (B,
 *   Q, max_faces) alone (about 1024 workgroups, a slice of at least VPN_WINDING_MIN_SLICE faces but for the last, at most
 *   VPN_WINDING_MAX_SLICES slices), so a shape always adds in the same order.
 * vpn_voliou_accumulate: two launches (one workgroup per sample, then ONE workgroup for the bookkeeping).  occ_pred, occ_gt
 *   uint8 [B,Q] (non-zero = inside); class_index int32 [B].  Writes counts int32 [B,4] = (I = #and, U = #or, Np, Ng) and rows
 *   fp32 [B,VPN_VOLIOU_WIDTH] = (iou I / U, precision I / Np, recall I / Ng, vol_pred Np / Q, vol_gt Ng / Q), each quotient
 *   formed in fp64 from the integers and rounded once, 0 where its denominator is 0.
 *   state: vpn_voliou_state_size(C) bytes (0: rejected sizes), 8-byte aligned, ZEROED BY THE CALLER before the first batch of
 *   an epoch: (1 + C) W doubles -- total[W], then class_sum[C][W] -- followed by 4 + C int64 -- n_samples, n_batches, n_empty
 *   (samples with U = 0), n_invalid, class_n[C].  Sums in sample order in fp64, totals SAMPLE-weighted, a class index outside
 *   [0, C) enters the totals and n_invalid only, two states merge by adding: the rules of vpn_surfeval_accumulate.
 * Nothing is allocated, no host synchronisation, no atomics, capturable, bit-equal from run to run.  A null pointer (xforms
 * may be NULL; occ / owner and w / occ as said), a non-positive size, one offset table without the other, max_faces outside 1 ..
 * F in the ragged layout, a workspace that is short or misaligned, a misaligned state: VPN_E_BADARG.  B > 65535, Q, P, F or C
 * above VPN_OCCUPANCY_MAX_ITEMS, K > VPN_MAX_PRIMS: VPN_E_TOOBIG.  All before any HIP call.  Added without a change of
 * VPN_ABI_VERSION. */
#define VPN_OCCUPANCY_TILE 256           /* queries per workgroup */
#define VPN_OCCUPANCY_MAX_ITEMS 16777216
#define VPN_WINDING_MIN_SLICE 128        /* a face slice of the winding scan has at least this many faces (but for the last) */
#define VPN_WINDING_MAX_SLICES 64
#define VPN_VOLIOU_WIDTH 5
int vpn_occupancy_prims(const float* params, const int32_t* kinds, const float* queries, int shared_queries, int B, int K, int Q,
                        uint8_t* occ, int32_t* owner, void* stream);
int vpn_winding_plan(int B, int Q, int max_faces, int* slice_faces);
size_t vpn_winding_workspace(int B, int Q, int F, int ragged, int max_faces);
int vpn_winding_number(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                       const float* xforms, const float* queries, int shared_queries, int B, int Q, int P, int F, int max_faces,
                       void* workspace, size_t workspace_bytes, float* w, uint8_t* occ, void* stream);
size_t vpn_voliou_state_size(int num_classes);
int vpn_voliou_accumulate(const uint8_t* occ_pred, const uint8_t* occ_gt, const int32_t* class_index, int B, int Q, int num_classes,
                          void* state, float* rows, int32_t* counts, void* stream);

/* ---- outer-surface extraction (csrc/isosurface.hip): the implicit field of a primitive assembly, and surface
 * nets on a lattice: ONE closed mesh per sample from a field, of a size that depends on the data.  DEVICE pointers.
 * vpn_primitive_field: one launch.  params, kinds, queries, shared_queries as vpn_occupancy_prims reads them.  f fp32 [B,Q] =
 *   min_k (m_k - 1) with m_k exactly as vpn_occupancy_prims forms it, so (f <= 0) is its occ bit for bit; a primitive whose
 *   m_k is a NaN is skipped, +inf when no primitive is left.
 * vpn_isosurface: four launches (count, scan, vertices, faces).  field fp32 [B,Nz,Ny,Nx], node (iz Ny + iy) Nx + ix; cx [Nx],
 *   cy [Ny], cz [Nz] fp32 node coordinates, strictly increasing (the caller's word: they are not read on the host).
 *   s = field - level, NaN -> +FLT_MAX, clamped to +-FLT_MAX; a node is inside iff s <= 0.  Cell (cx,cy,cz) has index (cz (Ny-1)
 *   + cy) (Nx-1) + cx and is active iff its 8 corners are neither all inside nor all outside.
 *   verts fp32 [B,max_verts,3]: the vertex of an active cell is the mean of the crossing points of its sign-changing edges, taken
 *     in the order axis x, y, z and within an axis by the offsets (0,0), (1,0), (0,1), (1,1) along the two other axes in cyclic
 *     order (x: y z, y: z x, z: x y); on edge a -> b the point is c_a + t (c_b - c_a) with t = s_a / (s_a - s_b) along the axis
 *     and the node coordinates on the other two; the sum in fp32 in that order, then divided by the count.  A vertex's number is
 *     the rank of its cell among the sample's active cells in cell-index order.
 *   faces int32 [B,max_faces,3], MESH-LOCAL: a sign-changing lattice edge with four cells around it gives the quad of their
 *     vertices, the cells counter-clockwise seen from the edge's positive direction (offsets (-,-), (0,-), (0,0), (-,0) in the
 *     cyclic plane), as triangles (c0,c1,c2), (c0,c2,c3) when the edge runs from inside to outside and with c1 and c3 swapped
 *     otherwise: counter-clockwise seen from outside, the convention of vpn_winding_number.  The quad belongs to the cell whose
 *     minimum corner is the edge's first node; faces are ordered by owner cell, then axis, then the two triangles.
 *   counts int32 [B,4] = (n_verts, n_faces, n_open, overflow).  n_open: the sign-changing edges in the six boundary faces of the
 *     lattice, which give no face; 0 means the mesh is closed.  Rows past the counts are written as 0 / (0,0,0): a padding face
 *     has no area.  n_verts > max_verts or n_faces > max_faces: overflow = 1, the true counts, every row of the sample padding.
 *   workspace: at least vpn_isosurface_workspace(B, Nx, Ny, Nz) bytes (0: rejected shapes), 16-byte aligned.
 * Nothing is allocated, no host synchronisation, no atomics, capturable, bit-equal from run to run.  A null pointer, a
 * non-positive size, a dimension below 2, a level that is not finite, a workspace that is short or misaligned: VPN_E_BADARG.
 * B > 65535, Q, Nx Ny Nz, max_verts or max_faces above VPN_OCCUPANCY_MAX_ITEMS, K > VPN_MAX_PRIMS: VPN_E_TOOBIG.  All before any
 * HIP call.  Added without a change of VPN_ABI_VERSION. */
int vpn_primitive_field(const float* params, const int32_t* kinds, const float* queries, int shared_queries, int B, int K, int Q,
                        float* f, void* stream);
size_t vpn_isosurface_workspace(int B, int Nx, int Ny, int Nz);
int vpn_isosurface(const float* field, const float* cx, const float* cy, const float* cz, float level, int B, int Nx, int Ny, int Nz,
                   int max_verts, int max_faces, void* workspace, size_t workspace_bytes, float* verts, int32_t* faces,
                   int32_t* counts, void* stream);

/* ---- occupancy loss (csrc/occloss.hip): the soft union of a primitive assembly against occupancy labels at
 * query points, with an overlap penalty, differentiable to the parameters.  DEVICE pointers.  params fp32 [B,K,VPN_PARAM_STRIDE],
 * kinds int32 [K], queries fp32 [Q,3] (shared_queries != 0) or [B,Q,3], read as vpn_primitive_field reads them (a sample stride
 * of 0: repeating a shared set B times gives the same bits).  labels [B,Q]: uint8 (labels_u8 != 0; non-zero = 1, what
 * vpn_occupancy_prims and vpn_winding_number write) or fp32 in [0,1] (the range is the caller's word).  tau: finite, > 0.
 *   per primitive   x~ = R^T (x - t) / v and m_k exactly as vpn_primitive_field forms them; d_k = m_k - 1, z_k = -d_k / tau, each
 *                   operation in fp32 and rounded by itself.  A primitive whose m_k is not finite (NaN or inf) is left out of
 *                   everything below, for that query.
 *   union logit     l = logsumexp_k z_k = zmax + log sum_k exp(z_k - zmax) (formed online, primitive by primitive: the running sum
 *                   is rescaled by exp(old max - new max) when the maximum grows); -inf when no primitive is left or every z_k is
 *                   -inf, +inf when a z_k is.  The soft occupancy is sigmoid(l).
 *   overlap sum     s = sum_k sigmoid(z_k), sigmoid(z) = 1 / (1 + exp(-z)) for z >= 0 and exp(z) / (1 + exp(z)) below.
 *   per query       bce = softplus(l) - y l with softplus(l) = max(l, 0) + log1p(exp(-|l|));  ov = relu(s - 1)^2.
 *   out [2]         (sum bce, sum ov) / (B Q).
 *   skipped         a query with a coordinate that is not finite, a NaN label, or an l that is not finite adds 0 to both sums and
 *                   to every gradient and 1 to n_skipped; the divisor stays B Q.
 * vpn_occloss_fwd: two launches (one work-item per (query, sample) with the records of 256 primitives at a time in LDS and one
 *   row of sums per workgroup -- xor tree over the wave, the four waves (0 + 1) + (2 + 3) --; then ONE workgroup that adds the
 *   rows in fp64: lane t rows t, t + 256, ... ascending, the lanes by a tree).  lse [B,Q] = l and s [B,Q], both or neither (NULL:
 *   not written): all the backward needs.  out [2] and n_skipped int32 [1] (may be NULL; saturates at INT_MAX); out NULL: the soft
 *   occupancy alone, one launch, labels and workspace are not used and n_skipped must be NULL.  lse or out must be given.
 * vpn_occloss_bwd: two launches.  grad DEVICE fp32 [2], first order:
 *     c_k = (grad[0] (sigmoid(l) - y) exp(z_k - l) + grad[1] 2 relu(s - 1) sigmoid(z_k) (1 - sigmoid(z_k))) / (B Q)
 *     (B Q is the exact product in fp64 in both calls: each of the two query factors of c_k is divided by it in fp64 and rounded once)
 *     dL/dm_k = -c_k / tau;  dm/dx~ = 2 x~ (sphere) or sign(x~_a) e_a with a the LOWEST axis attaining max |x~_i| and sign(0) = 0
 *     with gamma = dL/dx~ summed over the queries of (b, k):  dL/dt = -R (sum gamma / v),  dL/dv_i = -sum gamma_i x~_i / v_i,
 *     dL/dR[j][i] = sum gamma_i d_j / v_i with d = x - t = R (v o x~), and dL/dR -> q by the sampler's chain rule (the half-angle
 *     map of q3 included).  Twelve sums a primitive: sum gamma [3] and sum gamma_i x~_l [3][3].
 *   One workgroup per (query slice, sample); a lane keeps its slice's queries in registers, accumulates the twelve sums of a
 *   primitive over them in fp32, the wave adds them by the xor tree and writes a row; then per (b, k) the rows are added in fp64
 *   in ascending (slice, wave) order, the chain rule is applied in fp64 up to dL/dR and dparams [B,K,VPN_PARAM_STRIDE] is written
 *   whole.  A primitive with an extent that is 0 or not finite, or a t or a rotation that is not finite, has no finite m_k at any
 *   query: its row of dparams is 0.  No gradient to queries or labels.  lse and s as the forward wrote them for the same inputs.
 * vpn_occloss_plan returns the number of query slices (or a negative code) and writes the queries per slice = 256 qpl: qpl is the
 *   largest of 8, 4, 2, 1 that still gives VPN_OCCLOSS_MIN_GROUPS workgroups (else 1), a function of (B, Q) alone, so a shape
 *   always adds in the same order.
 * workspace: at least vpn_occloss_workspace(B, K, Q) bytes (0: rejected shapes), 16-byte aligned; it serves either call.
 * Nothing is allocated, no host synchronisation, no atomics, capturable, bit-equal from run to run.  A null pointer (but for
 * those said to be optional), a non-positive size, lse without s, neither lse nor out, n_skipped without out, a tau that is not
 * finite or not > 0, a workspace that is short or misaligned: VPN_E_BADARG.  B > 65535, Q > VPN_OCCUPANCY_MAX_ITEMS, K >
 * VPN_MAX_PRIMS: VPN_E_TOOBIG.  All before any HIP call.  Added without a change of VPN_ABI_VERSION. */
#define VPN_OCCLOSS_MAX_QPL 8            /* queries a lane of the backward keeps in registers, at most */
#define VPN_OCCLOSS_MIN_GROUPS 256       /* the backward halves its slice until it launches this many workgroups */
int vpn_occloss_plan(int B, int Q, int* slice_queries);
size_t vpn_occloss_workspace(int B, int K, int Q);
int vpn_occloss_fwd(const float* params, const int32_t* kinds, const float* queries, int shared_queries, const void* labels,
                    int labels_u8, int B, int K, int Q, float tau, void* workspace, size_t workspace_bytes, float* lse, float* s,
                    float* out, int32_t* n_skipped, void* stream);
int vpn_occloss_bwd(const float* grad, const float* params, const int32_t* kinds, const float* queries, int shared_queries,
                    const void* labels, int labels_u8, const float* lse, const float* s, int B, int K, int Q, float tau,
                    void* workspace, size_t workspace_bytes, float* dparams, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPN_HIP_H */
