/*
 * thermal_nerf_hip.h -- C ABI of libthermal_nerf_hip.so (MI355X / gfx950).
 *
 * The reference (yvette256/nerfstudio-thermal) has no FFI of its own: its native arithmetic enters
 * through the Python objects of tinycudann (tcnn.Encoding / tcnn.Network / tcnn.NetworkWithInputEncoding)
 * and, on the CPU path that is this project's oracle, through ATen.  Each entry point below replaces one
 * such seam; the reference location it stands in for is cited as (file:line), relative to
 * /root/reference/nerfstudio/.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *  - plain C: device pointers + sizes + an opaque stream handle (a hipStream_t passed as void*; NULL = default stream).
 *  - every function returns 0 on success or a negative TN_E* code; nothing throws, nothing allocates or frees
 *    caller memory, nothing synchronises the device.  Work is enqueued on `stream`.
 *  - all float tensors are fp32, contiguous, row-major; sample tensors are dense [N, S] per level
 *    (N rays, S samples; "bins" tensors are [N, S+1]).
 *  - operand-shape violations are rejected on the host (TN_EINVAL) before anything is launched.
 *
 * State and environment (everything the library keeps or reads besides its arguments):
 *  - Process-wide state: ONE map of companion streams -- a second HIP stream (+ two events) per (device, caller stream), created the first time
 *    an entry point forks work beside the caller's stream (tn_field_bwd*: k_field_dpos beside the table scatter) and kept for the life of the
 *    process; tn_shutdown() waits for them and destroys them (they are re-created on demand).  The last error string (tn_last_error) is
 *    per process too.  There is no other hidden state: no context object, no caches, no allocations -- workspaces are the caller's.
 *    (SURVEY.md 8b proposed tn_create / tn_destroy around an opaque context; with the state reduced to this map a context would own nothing
 *    else, so the teardown is the one call.)
 *  - The data-parallel gradient exchange: the Python package uses torch.distributed over RCCL on slices of the caller's gradient arena
 *    (nerfstudio_thermal_amd/parallel.py), exactly where the reference has torch DDP; tn_comm_* / tn_allreduce_grads offer the same exchange to a
 *    host that binds only this ABI (RCCL resolved at run time, no link-time dependency).
 *  - Environment switches, read once per process, all tuning / diagnostic aids whose defaults are the product path:
 *      TN_NO_FORK=1               no companion streams (everything on the caller's stream)
 *      TN_SCATTER_MODE=2|1|0      table-gradient scatter: 2 = segmented (default: block-private record regions, no global atomics), 1 = binned
 *                                 (rounds 2-5: per-bucket arrays with reservations), 0 = the round-1 global-atomic scatter with dense replicas.
 *                                 Read on every call; the bin and fold launches of one backward must see the same value.
 *      TN_SCATTER_REPLICAS=n, TN_SCATTER_SPARSE_CHUNK=n, TN_SCATTER_MERGE_RES=n      tuning knobs of the two scatter paths
 *      TN_FOLD_TRACE=1 [TN_FOLD_TRACE_FILE=path]   per-block timing of the fold pass (synchronises and prints: diagnostics only)
 *      TN_BIN_LEVEL_GROUPS=n      force the number of level groups of the bin pass (diagnostic: n = levels -> one level per block)
 *      TN_DPOS_COWORK=0           (read per call) the main field's d position pass as a launch of its own (forked with TN_BWD_FORK_DPOS) instead of
 *                                 extra blocks of the table scatter's bin launch
 *      TN_POSE_FINISH_COWORK=0    (read per call) tn_train_step's last backward launch (tn_pose_bwd_finish_check) always as a launch of its own instead of
 *                                 the first blocks of the main grid's fold launch on iterations without a proposal update
 *      TN_FOLD_ADAM=0             tn_train_step: the main grid's fold never steps its own table (A/B timing, tests).  By default the fold block that has
 *                                 summed a bucket's gradient in LDS applies Adam to the bucket's slots itself -- the table gradient is neither stored,
 *                                 read back nor zeroed, the Adam launch skips the table -- whenever the segmented scatter runs with one fold block per
 *                                 bucket (<= 524288 field samples), table_grad_is_zero holds, the d position pass rides in the bin launch and one
 *                                 optimiser range contains the table; and, decided on the device every iteration, max |d enc| <= FLT_MAX / (8 P).  Same
 *                                 results; slots 12..15 of losses16 then hold max |d enc|, the decision (0 not armed, 1 fused, 2 fell back), and the
 *                                 step's two scalars
 *      TN_FUSE_RENDER=1           (read per call) tn_train_step with tn_render_fwd / tn_train_losses / tn_render_bwd as ONE launch,
 *                                 tn_render_losses_bwd -- a measured experiment that is correct and not faster (profiles/r05_experiments.md)
 *      TN_NEXT_SAMPLING=0|2|3|4   (read per call) tn_train_step's next_sampling: 0 = never taken (every iteration samples in line); 2 = the chain as a launch
 *                                 of its own behind the optimiser launch; 3 = on a companion stream beside it (A/B timing aids: same results);
 *                                 4 = (opt-in experiment) the chain's waves also step most of the field's optimiser range themselves, between
 *                                 their stages, through LDS-staged asynchronous loads: same forward buffer bit for bit, the same Adam
 *                                 arithmetic; the launch 141 -> 132 us (profiles/r06_next_sampling.md).  TN_FUSED_SITES=<n> sizes its share
 *      TN_HEAD_BF16X3=1           (read per call; opt-in experiment, never the default) the colour head's two 64-wide layers in tn_field_fwd /
 *                                 tn_field_bwd* on split-bf16 matrix instructions: x = hi + lo in bf16, three v_mfma_f32_32x32x16_bf16 per
 *                                 product, fp32 accumulators (~2^-16 relative).  The density path stays fp32 bit for bit.  RGB / thermal agree
 *                                 with the fp32 path to ~1e-5; tests/test_head_bf16x3_gpu.py, bench.py extra.head_bf16x3
 *    The Python package reads TN_FUSE_SMALL=0 (one launch per reference seam instead of the fused small kernels: test aid), TN_DM_PREFETCH=0 (the
 *    device data manager launches every batch itself instead of handing the next one to tn_train_step: A/B timing), TN_NEXT_SAMPLING=0 (the engine
 *    plans no next_sampling), TN_DP_SCHEDULE=overlapped|simple (pins the data-parallel exchange schedule of trainer.FusedTrainerMixin) and writes
 *    nothing into the environment (rounds 2-4 set GPU_MAX_HW_QUEUES=8 at import: the schedules now fit the runtime's default of four).
 */
#ifndef THERMAL_NERF_HIP_H
#define THERMAL_NERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported (tests/test_abi_cpu.py compares `nm -D`). */
#if defined(__GNUC__) || defined(__clang__)
#define TN_API __attribute__((visibility("default")))
#else
#define TN_API
#endif

#define TN_OK 0
#define TN_EINVAL (-22)   /* bad argument / unsupported shape */
#define TN_ELAUNCH (-5)   /* hipLaunch / runtime error (see tn_last_error) */
#define TN_MAX_LEVELS 16
#define TN_MAX_SAMPLES 256 /* samples per ray per level (one 64-lane wave x 4) */

typedef void* tn_stream_t;

/* Multiresolution hash grid as the reference's torch HashEncoding lays it out
 * (field_components/encodings.py:343-347,377-379): table [num_levels * 2^log2_hashmap_size, 2]. */
typedef struct TnGrid {
  const float* table;
  float* table_grad; /* may be NULL when no gradient is wanted */
  int32_t num_levels;
  int32_t log2_hashmap_size;
  float res[TN_MAX_LEVELS]; /* floor(min_res * growth^l) as fp32, computed by the host exactly as the reference does */
  /* NULL, or one float on the device that every table-gradient scatter of this grid sets to 1.0f when an entry of table_grad comes out inf / NaN
   * (GradScaler's found_inf for the optimiser group that owns the table, engine/trainer.py:470-495 -> torch/amp/grad_scaler.py: raised by the
   * kernel that writes the final value, so no separate pass over the 64 MB of table gradient is needed; never cleared by the scatter) */
  float* nonfinite_flag;
  /* The caller's PROMISE (not checked): every entry of table_grad is zero when a table-gradient scatter of this grid starts, and this scatter is
   * the only writer of table_grad until it ends.  The fold pass then STORES a slot's sum instead of adding it to what the slot holds (no read of
   * the 64 MB before the write: the main grid's scatter 159 -> 147 us).  A trainer whose optimiser launch clears the gradients behind its read
   * (tn_adam_step_ranges_amp(zero_grads)) and scatters once per table and iteration may set it; gradient accumulation over several backward
   * passes, or two scatters into one table (separate density fields with the density loss), must leave it 0. */
  int32_t table_grad_is_zero;
} TnGrid;

/* HashMLPDensityField (fields/density_fields.py:34-118): 5 lvl x 2 feat -> Linear(10,16) ReLU Linear(16,1). */
typedef struct TnPropNet {
  TnGrid grid;
  const float *w0, *b0, *w1, *b1; /* [16,10] [16] [1,16] [1] as nn.Linear stores them */
  float *gw0, *gb0, *gw1, *gb1;   /* gradient accumulators, may be NULL */
} TnPropNet;

/* ThermalNerfactoField (fields/thermal_nerfacto_field.py:37-99 over fields/nerfacto_field.py:73-202):
 * 16 lvl x 2 feat -> Linear(32,64) ReLU Linear(64,16); head Linear(63,64) ReLU Linear(64,64) ReLU Linear(64,C) sigmoid. */
typedef struct TnField {
  TnGrid grid;
  const float *w0, *b0, *w1, *b1;             /* [64,32] [64] [16,64] [16] */
  const float *hw0, *hb0, *hw1, *hb1, *hw2, *hb2; /* [64,63] [64] [64,64] [64] [C,64] [C] */
  const float* emb;                            /* [num_images, 32] appearance embedding */
  float *gw0, *gb0, *gw1, *gb1, *ghw0, *ghb0, *ghw1, *ghb1, *ghw2, *ghb2, *gemb; /* gradients, may be NULL */
  int32_t num_channels; /* C: 4 (shared RGBT), 3 or 1 (separate) */
  int32_t num_images;
} TnField;

TN_API const char* tn_last_error(void);
TN_API int tn_version(void);
/* bytes of device scratch tn_field_* need for `num_points` samples (packed weights + saved activations). */
TN_API int64_t tn_field_workspace_bytes(int64_t num_points, int32_t training);
/* Work plan of the field's hash-grid gather (HashEncoding.pytorch_fwd, field_components/encodings.py:401-461), for tests and diagnostics.
 * The gather is XCD-affine: workgroup b runs on XCD b % 8 and reads ONE level, so that a hashed level's table is served from that XCD's L2;
 * XCD x runs level x for all samples, then level x + 8.  out [8][2][3] int32: item i of XCD x = {level (-1: unused), first chunk,
 * chunk count}.  Returns the number of chunks per level (every level's chunks appear exactly once in the plan) or TN_EINVAL. */
TN_API int32_t tn_field_encode_plan(const TnGrid* grid, int64_t num_points, int32_t* out);

/* ---- N2  PatchPixelSampler.sample on a jagged image list + ground-truth gather (data/pixel_samplers.py:296-337 collate_image_dataset_batch_list,
 *          :389-441 PatchPixelSampler.sample_method without masks; what VanillaDataManager.next_train does on the host every step,
 *          data/datamanagers/base_datamanager.py:538-547).  The cached training images stay resident in HBM:
 * images: all images back to back, image i is [height[i], width[i], 3] fp32 starting at float offset image_offsets[i];
 * is_thermal [num_images] fp32 by batch position; image_idx [num_images] int64 = dataset (camera) index of each batch position;
 * u [num_rays / patch^2, 3] fp32 uniforms in [0,1) -- exactly what torch.rand returns in the reference, image after image (column 0 unused).
 * Every image gets (num_rays / num_images) / patch^2 patches and the last one the remainder, which must be a whole number of patches
 * (the reference asserts the same).  patch_size 1..8.
 * Outputs: ray_indices [N,3] int64 (camera,row,col), image [N,3], is_thermal_out [N], camera_indices [N] int64 (= ray_indices[:,0] as the
 * contiguous vector the field kernels take; may be NULL). */
TN_API int tn_sample_pixels(const float* images, const int64_t* image_offsets, const int32_t* heights, const int32_t* widths,
                     const float* is_thermal, const int64_t* image_idx, int32_t num_images, const float* u, int64_t num_rays,
                     int32_t patch_size, int64_t* ray_indices, float* image, float* is_thermal_out, int64_t* camera_indices,
                     tn_stream_t stream);

/* ---- a1  RayGenerator.forward -> Cameras._generate_rays_from_coords (model_components/ray_generators.py:40-55,
 *          cameras/cameras.py:598-655,781-786,886-909; undistortion cameras/camera_utils.py:409-446).
 * ray_indices [N,3] int64 (camera,row,col); c2w [C,3,4]; fx,fy,cx,cy [C]; distortion [C,6] (k1,k2,k3,k4,p1,p2) or NULL. */
TN_API int tn_raygen(const int64_t* ray_indices, const float* c2w, const float* fx, const float* fy, const float* cx,
              const float* cy, const float* distortion, int32_t num_cameras, int64_t N, float* origins, float* directions,
              float* pixel_area, float* directions_norm, tn_stream_t stream);
/* N2 + a1 in ONE launch (VanillaDataManager.next_train, data/datamanagers/base_datamanager.py:538-547: pixel sampler -> ground truth ->
 * RayGenerator): arguments of tn_sample_pixels followed by those of tn_raygen without ray_indices (the sampled pixel is handed over in
 * registers; ray_indices is still written).  Same results as the two calls. 
 * pixel_area may be NULL (a trainer whose model does not read it: the two extra undistortions per ray that only serve it are skipped). */
/* The arguments of tn_sample_rays as a block: TnTrainStep::next_sample hands the NEXT iteration's batch to tn_train_step, which samples it in
 * co-work blocks of its optimiser launch (the last launch of the iteration: an HBM-bound pass beside a short, latency-bound one). */
typedef struct TnSampleRays {
  const float* images; const int64_t* image_offsets; const int32_t* heights; const int32_t* widths; const float* is_thermal; const int64_t* image_idx;
  int32_t num_images; const float* u; int64_t num_rays; int32_t patch_size;
  int64_t* ray_indices; float* image; float* is_thermal_out; int64_t* camera_indices;
  const float* c2w; const float* fx; const float* fy; const float* cx; const float* cy; const float* distortion; int32_t num_cameras;
  float* origins; float* directions; float* pixel_area; float* directions_norm;
} TnSampleRays;
TN_API int tn_sample_rays_args(const TnSampleRays* args, tn_stream_t stream); /* tn_sample_rays on the block */
TN_API int tn_sample_rays(const float* images, const int64_t* image_offsets, const int32_t* heights, const int32_t* widths,
                   const float* is_thermal, const int64_t* image_idx, int32_t num_images, const float* u, int64_t num_rays,
                   int32_t patch_size, int64_t* ray_indices, float* image, float* is_thermal_out, int64_t* camera_indices,
                   const float* c2w, const float* fx, const float* fy, const float* cx, const float* cy, const float* distortion,
                   int32_t num_cameras, float* origins, float* directions, float* pixel_area, float* directions_norm, tn_stream_t stream);

/* ---- a4  CameraOptimizer(SO3xR3).apply_to_raybundle (cameras/camera_optimizers.py:130-176, cameras/lie_groups.py:24-58).
 * pose_adjustment [C,6]; frozen [C] uint8 (1 = non-trainable camera -> identity); camera_indices [N] int64. */
TN_API int tn_pose_apply_fwd(const float* pose_adjustment, const uint8_t* frozen, const int64_t* camera_indices, const float* origins_in,
                      const float* directions_in, int64_t N, int32_t num_cameras, float* origins_out, float* directions_out,
                      tn_stream_t stream);
/* backward: d_origins/d_directions [N,3] -> accumulates into grad_pose [C,6]. */
TN_API int tn_pose_apply_bwd(const float* pose_adjustment, const uint8_t* frozen, const int64_t* camera_indices, const float* directions_in,
                      const float* d_origins, const float* d_directions, int64_t N, int32_t num_cameras, float* grad_pose,
                      tn_stream_t stream);
/* CameraOptimizer("shared_SO3xR3").apply_to_raybundle (cameras/camera_optimizers.py:108-117,150-163): ONE row shared_row [6] corrects every
 * camera that is not frozen: origins_out = origins_in + t, directions_out = R directions_in with [R | t] = exp_map_SO3xR3(shared_row), the
 * identity where frozen[camera] is set (frozen may be NULL: no camera is).  One launch; the exp map is evaluated once per block, with the device
 * function tn_pose_apply_fwd uses per ray, so the result equals tn_pose_apply_fwd's on the row tiled to [C,6] bit for bit.  A camera index
 * outside [0, C) reads camera 0's flag, as in tn_pose_apply_fwd.  N == 0: TN_OK, nothing is touched.  N outside [0, 2^32], num_cameras outside
 * [1, 2^20] or a NULL pointer: TN_EINVAL before any launch. */
TN_API int tn_pose_shared_apply(const float* shared_row, const uint8_t* frozen, const int64_t* camera_indices, const float* origins_in,
                         const float* directions_in, int64_t N, int32_t num_cameras, float* origins_out, float* directions_out,
                         tn_stream_t stream);
/* backward of tn_pose_shared_apply, optionally through a per-camera correction applied on top of it (d2 = R_c d1, o2 = o1 + t_c):
 * d_origins / d_directions [N,3] = the gradient of the rays the render saw; directions_in [N,3] = the directions tn_pose_shared_apply was
 * given; pose_adjustment [C,6] = the per-camera rows applied behind it, or NULL (R_c = I: per-camera optimiser off, or an eval render).
 *   grad_row[0:3] += sum d_origins,   grad_row[3:6] += sum J(shared_row; directions_in)^T (R_c^T d_directions)   over the rays of cameras
 * that are not frozen (J: the derivative tn_pose_apply_bwd uses).  Deterministic: one launch sums per wave and per block, in double, into
 * workspace (tn_pose_shared_bwd_workspace_bytes(N) bytes), a second single-block launch adds the blocks' sums in block order, in double, and
 * adds the result to grad_row [6]; no floating-point atomics, the same inputs give the same bits.  With every camera frozen grad_row keeps
 * its bits; N == 0: TN_OK, nothing is touched.  Range and pointer checks as tn_pose_shared_apply, plus a short workspace: TN_EINVAL before
 * any launch.  GradScaler's found_inf: this entry point raises no flag -- the shared rows' optimiser groups are covered by the range check
 * over the gradient arena (tn_grad_nonfinite_ranges), which the engine runs whenever a shared row is trained.  The regulariser of a shared
 * row and its gradient: tn_camera_reg with num_cameras = 1. */
TN_API int64_t tn_pose_shared_bwd_workspace_bytes(int64_t N);
TN_API int tn_pose_shared_bwd(const float* shared_row, const uint8_t* frozen, const int64_t* camera_indices, const float* directions_in,
                       const float* d_origins, const float* d_directions, const float* pose_adjustment, int64_t N, int32_t num_cameras,
                       void* workspace, int64_t workspace_bytes, float* grad_row, tn_stream_t stream);

/* ---- a6  UniformLinDispPiecewiseSampler / SpacedSampler.generate_ray_samples (model_components/ray_samplers.py:78-128,225-248).
 * lin_bins [S+1] = torch.linspace(0,1,S+1) supplied by the host; jitter [N] or NULL (eval). Outputs s_bins,e_bins [N,S+1]. */
TN_API int tn_spaced_bins(const float* lin_bins, const float* jitter, const float* nears, const float* fars, int64_t N, int32_t S,
                   float* s_bins, float* e_bins, tn_stream_t stream);
/* tn_pose_apply_fwd and tn_spaced_bins (the two independent first steps of a training render) in one launch; arguments of the former, then of
 * the latter without N. */
TN_API int tn_pose_spaced_bins(const float* pose_adjustment, const uint8_t* frozen, const int64_t* camera_indices, const float* origins_in,
                        const float* directions_in, int64_t N, int32_t num_cameras, float* origins_out, float* directions_out,
                        const float* lin_bins, const float* jitter, const float* nears, const float* fars, int32_t S, float* s_bins,
                        float* e_bins, tn_stream_t stream);

/* ---- a8/a9/a10  Field.density_fn -> HashMLPDensityField.get_density (fields/base_field.py:48-68, fields/density_fields.py:95-118,
 *          field_components/encodings.py:401-461, field_components/mlp.py:159-178, field_components/activations.py:28-41).
 * positions = origins + directions * (e_bins[s]+e_bins[s+1])/2 (cameras/rays.py:49-58). density [N,S]. */
TN_API int tn_prop_density_fwd(const TnPropNet* net, const float* origins, const float* directions, const float* e_bins, int64_t N,
                        int32_t S, float* density, tn_stream_t stream);
/* backward of the above: d_density [N,S] -> table/MLP gradients (accumulated) and, if non-NULL, d_origins/d_directions [N,3] (accumulated).
 * workspace: tn_prop_workspace_bytes(N*S) bytes of device scratch (d enc for the table scatter + the scatter's records); workspace_bytes = the size
 * of the buffer behind it: a shorter one is refused with TN_EINVAL (every workspace_bytes argument below works the same way -- the scratch of
 * a backward pass is hundreds of MB, and a short buffer would be a device out-of-bounds write the callee could not see). */
TN_API int64_t tn_prop_workspace_bytes(int64_t num_points);
TN_API int tn_prop_density_bwd(const TnPropNet* net, const float* origins, const float* directions, const float* e_bins,
                        const float* d_density, int64_t N, int32_t S, void* workspace, int64_t workspace_bytes, float* d_origins,
                        float* d_directions, tn_stream_t stream);

/* ---- a9 (backward)  autograd of HashEncoding.pytorch_fwd (field_components/encodings.py:420-461) with respect to the table (and the sample
 *          position): trilinear scatter-add of g_enc [N*S, ld] (feature 2*level + f) into grid->table_grad; d_origins/d_directions optional.
 *          ld == -1: g_enc is LEVEL-major, [num_levels][N*S][2] (what the main field's backward produces: coalesced reads per level).
 *          Used by tn_prop_density_bwd and tn_field_bwd; exposed because it is the dominant kernel of the training step.
 *          workspace: tn_hash_scatter_workspace_bytes(N*S, num_levels) of 256-byte-aligned device scratch (contents irrelevant), or NULL.
 *          With it the scatter is atomic-free: every contribution is written once as a (slot, value) record into the bucket of its
 *          2^12-slot table slice and the buckets are summed in LDS (coarse levels are pre-merged in registers); NULL adds every
 *          contribution straight into table_grad with global float atomics (same result up to summation order, several times slower). */
TN_API int64_t tn_hash_scatter_workspace_bytes(int64_t num_points, int32_t num_levels);
TN_API int tn_hash_scatter(const TnGrid* grid, const float* origins, const float* directions, const float* e_bins, const float* g_enc, int32_t ld,
                    int64_t N, int32_t S, float* d_origins, float* d_directions, void* workspace, int64_t workspace_bytes, tn_stream_t stream);

/* ---- a11 RaySamples.get_weights (cameras/rays.py:128-150) and, optionally, DepthRenderer("median") of the same level
 *          (model_components/renderers.py:547-557; used for prop_depth_i, models/nerfacto.py:351-352). median_depth may be NULL. */
TN_API int tn_weights_fwd(const float* e_bins, const float* density, int64_t N, int32_t S, float* weights, float* median_depth,
                   tn_stream_t stream);
TN_API int tn_weights_bwd(const float* e_bins, const float* density, const float* weights, const float* d_weights, int64_t N, int32_t S,
                   float* d_density, tn_stream_t stream);

/* ---- a7  PDFSampler.generate_ray_samples incl. the anneal pow of ProposalNetworkSampler (model_components/ray_samplers.py:276-372,602).
 * u_lin [S+1] = torch.linspace(0, 1-1/(S+1), S+1) supplied by the host (eval adds 1/(2(S+1)), train adds jitter/(S+1)). */
TN_API int tn_pdf_resample(const float* s_bins_prev, const float* weights_prev, int32_t S_prev, float anneal, const float* u_lin,
                    const float* jitter, const float* nears, const float* fars, int64_t N, int32_t S, float* s_bins, float* e_bins,
                    tn_stream_t stream);

/* a11 + a7 back to back, as ProposalNetworkSampler.generate_ray_samples always calls them (ray_samplers.py:593-611): the weights of the
 * previous level (written to weights_prev [N,S_prev]; median_prev [N] optional) and the bins of the next level, one launch, the weights
 * handed over in registers.  Bit-identical to tn_weights_fwd followed by tn_pdf_resample. */
TN_API int tn_weights_resample(const float* e_bins_prev, const float* density_prev, const float* s_bins_prev, int32_t S_prev, float anneal,
                        const float* u_lin, const float* jitter, const float* nears, const float* fars, int64_t N, int32_t S,
                        float* weights_prev, float* median_prev, float* s_bins, float* e_bins, tn_stream_t stream);

/* ---- a12/a13/a14  Field.forward = NerfactoField.get_density + get_outputs with ThermalNerfactoField.mlp_head
 *          (fields/base_field.py:114-133, fields/nerfacto_field.py:205-229,272-348, fields/thermal_nerfacto_field.py:91-99).
 * camera_indices [N] int64; training!=0 uses emb[camera], else mean(emb) (use_average_appearance_embedding=True).
 * Outputs: density [N,S], rgb [N,S,C], optional density_before_activation [N,S] (may be NULL).
 * workspace: device scratch of tn_field_workspace_bytes(N*S, training) bytes; when training!=0 it keeps the activations
 * tn_field_bwd consumes, so the same pointer must be passed to both. */
TN_API int tn_field_pack_weights(const TnField* field, void* workspace, tn_stream_t stream);
TN_API int tn_field_fwd(const TnField* field, const float* origins, const float* directions, const int64_t* camera_indices, const float* e_bins,
                 int64_t N, int32_t S, int32_t training, void* workspace, int64_t workspace_bytes, float* density, float* rgb,
                 float* density_pre, tn_stream_t stream);
/* backward: d_density [N,S], d_rgb [N,S,C] -> all TnField gradients (accumulated); d_origins/d_directions optional (accumulated).
 * d_rgb = NULL: density-only backward of tn_field_density_fwd(training != 0) (see there).
 * The appearance embedding's gradients (the embedding rows and the embedding columns of the head's first weight matrix) are formed from
 * per-camera sums kept in the workspace (head layer 0's bias gradient restricted to the camera; the training forward likewise adds a
 * per-camera vector instead of multiplying the embedding per sample): num_images <= TN_FIELD_MAX_IMAGES, refused with TN_EINVAL beyond.  The forward (training != 0) clears
 * those sums and the backward leaves them cleared: the workspace may come from an uninitialised allocation. */
#define TN_FIELD_MAX_IMAGES 4096
TN_API int tn_field_bwd(const TnField* field, const float* origins, const float* directions, const int64_t* camera_indices, const float* e_bins,
                 const float* d_density, const float* d_rgb, int64_t N, int32_t S, void* workspace, int64_t workspace_bytes, float* d_origins,
                 float* d_directions, tn_stream_t stream);
/* The same backward in phases, for data-parallel training: the table gradient of a level range is final as soon as its scatter has run,
 * so the caller can start that range's all-reduce (DDP's bucketed reducer, pipelines/base_pipeline.py:281-283) while the next range is
 * scattered.  phases is a bit set; tn_field_bwd == all three with levels [0, num_levels):
 *   TN_BWD_MLP      MLP backward + weight/bias/embedding gradients (the fused chain; the embedding's two gradients are finished from its
 *                   per-camera sums at the head of the d-position launch, or in a small launch of their own without one) and, when
 *                   d_origins is given, d position from the forward's saved
 *                   d enc / d offset (k_field_dpos); with TN_BWD_FORK_DPOS that second launch goes to a library-owned companion stream
 *                   beside the scatter -- worth it only when other streams are busy anyway (a second active queue costs more than it hides)
 *                   (when TN_BWD_MLP and a TN_BWD_SCATTER over all levels come in ONE call and the scatter takes its segmented path, the pass
 *                   gets no launch at all: it runs in extra blocks of the scatter's bin launch, d_origins / d_directions complete when that is)
 *   TN_BWD_SCATTER  table gradient of levels [level_begin, level_end); needs TN_BWD_MLP done
 *   TN_BWD_JOIN     make `stream` wait for the companion stream; required before d_origins / d_directions or the workspace are used again
 *   TN_BWD_SCATTER_BIN / TN_BWD_SCATTER_FOLD  the same scatter in its two passes: BIN writes the (slot, value) records of ALL levels once
 *                   (+ the d_origins/d_directions contribution); FOLD sums the records of levels [level_begin, level_end) into the table
 *                   gradient.  One BIN, then one FOLD per exchanged level range, costs the same as a single TN_BWD_SCATTER over all levels;
 *                   TN_BWD_SCATTER per range repeats the per-sample work of the bin pass for every range.
 *   TN_BWD_COUNTERS_CLEAN  with TN_BWD_SCATTER (whole grid) or TN_BWD_SCATTER_BIN in a call WITHOUT TN_BWD_MLP: the caller vouches that the
 *                   TN_BWD_MLP phase of this workspace and batch has run since the workspace's last scatter.  That launch leaves the bin
 *                   pass's bucket counters zeroed; without the flag a phase-by-phase backward pays a memset launch for them. */
enum { TN_BWD_MLP = 1, TN_BWD_SCATTER = 2, TN_BWD_JOIN = 4, TN_BWD_SCATTER_BIN = 8, TN_BWD_SCATTER_FOLD = 16, TN_BWD_FORK_DPOS = 32,
       TN_BWD_COUNTERS_CLEAN = 64 };
TN_API int tn_field_bwd_phase(const TnField* field, const float* origins, const float* directions, const int64_t* camera_indices,
                       const float* e_bins, const float* d_density, const float* d_rgb, int64_t N, int32_t S, void* workspace,
                       int64_t workspace_bytes, float* d_origins, float* d_directions, int32_t phases, int32_t level_begin, int32_t level_end,
                       tn_stream_t stream);
/* Caps the grid of the TN_BWD_MLP launch (k_field_bwd_fused: four waves per block, every wave walks a contiguous slab of 32-sample tiles) at
 * max_blocks blocks; max_blocks <= 0 restores the default, one block per CU.  Process-wide; returns the cap that was in force.  The results do
 * not depend on it beyond the order of the float sums.  For tests, which make a small batch walk several tiles per wave with it. */
TN_API int32_t tn_field_bwd_max_blocks(int32_t max_blocks);
/* Data-parallel exchange of the COARSE levels in dense form.  Levels whose (res+1)^3 cells are fewer than the table's slots are accumulated
 * in dense per-cell replicas anyway; their slice of the table gradient is almost all zeros (332 k possible non-zeros in 2.6 M slots for
 * levels 0-4 of the default grid), so a data-parallel run exchanges the per-cell sums (2.65 MB) instead of the table slice (20 MB):
 *   n = tn_field_dense_count(field, N*S, lb, le)      float2 cells of levels [lb, le) if ALL of them are dense levels for this batch size, else 0
 *   tn_field_bwd_scatter_dense(..., lb, le, dense_sum) as TN_BWD_SCATTER of that range, but the per-cell sums go to dense_sum [n,2] (written, not
 *                                                     accumulated) and the table gradient of the range is left untouched
 *   (all-reduce dense_sum)
 *   tn_field_dense_fold(field, N*S, lb, le, dense_sum) hashes the sums into the table gradient (accumulating), as the plain scatter would have. */
TN_API int64_t tn_field_dense_count(const TnField* field, int64_t num_points, int32_t level_begin, int32_t level_end);
TN_API int tn_field_bwd_scatter_dense(const TnField* field, const float* origins, const float* directions, const float* e_bins, int64_t N, int32_t S,
                               void* workspace, int64_t workspace_bytes, float* d_origins, float* d_directions, int32_t level_begin, int32_t level_end,
                               float* dense_sum, tn_stream_t stream);
TN_API int tn_field_dense_fold(const TnField* field, int64_t num_points, int32_t level_begin, int32_t level_end, const float* dense_sum,
                        tn_stream_t stream);
/* density only (cross-evaluation density2 / density2_thermal, models/thermal_nerfacto.py:447-458): get_density without get_outputs.
 * training != 0 keeps what the backward needs in `workspace` (sized with tn_field_workspace_bytes(N*S, 1)); that backward is
 * tn_field_bwd / tn_field_bwd_phase with d_rgb = NULL: the colour head, its three weight gradients and the appearance embedding are skipped. */
TN_API int tn_field_density_fwd(const TnField* field, const float* origins, const float* directions, const float* e_bins, int64_t N, int32_t S,
                         int32_t training, void* workspace, int64_t workspace_bytes, float* density, tn_stream_t stream);

/* ---- a15/a16  RGBRenderer / RGBTRenderer (background "last_sample"), AccumulationRenderer, DepthRenderer median+expected
 *          (model_components/renderers.py:118-133,238-245,292-307,418-425,509,547-576).
 * rgb [N,S,C]; outputs comp [N,C], accumulation [N], depth_median [N], depth_expected [N] (unclipped) and
 * steps_minmax [2] (running min/max of the sample midpoints as ordered uint32 bit patterns; initialise with tn_minmax_init,
 * then call tn_clip_depth to apply the batch-global clip of renderers.py:574). */
TN_API int tn_minmax_init(uint32_t* steps_minmax, tn_stream_t stream);
TN_API int tn_composite_fwd(const float* rgb, const float* weights, const float* e_bins, int64_t N, int32_t S, int32_t C, int32_t training,
                     float* comp, float* accumulation, float* depth_median, float* depth_expected, uint32_t* steps_minmax,
                     tn_stream_t stream);
TN_API int tn_clip_depth(float* depth_expected, const uint32_t* steps_minmax, int64_t N, tn_stream_t stream);
/* backward (train mode): d_comp [N,C] -> d_rgb [N,S,C] (written) and d_weights [N,S] (accumulated). */
TN_API int tn_composite_bwd(const float* rgb, const float* weights, const float* d_comp, int64_t N, int32_t S, int32_t C, float* d_rgb,
                     float* d_weights, tn_stream_t stream);

/* a11 + a15 + a16 of the last sampling level in ONE launch: RaySamples.get_weights (cameras/rays.py:128-150) followed by every renderer above
 * (models/nerfacto.py:330-340), the weights handed over in registers; a second small launch applies the batch-global clip of the expected
 * depth.  Results are bit-identical to tn_weights_fwd + tn_minmax_init + tn_composite_fwd + tn_clip_depth (two launches, not four, and no
 * atomics).  scratch: TN_RENDER_SCRATCH_FLOATS floats of device memory, contents irrelevant (required when depth_expected is given; one
 * buffer per stream that may run this concurrently).  accumulation / depth_median / depth_expected may be NULL. */
#define TN_RENDER_SCRATCH_FLOATS 4096
TN_API int tn_render_fwd(const float* e_bins, const float* density, const float* rgb, int64_t N, int32_t S, int32_t C, int32_t training,
                  float* weights, float* comp, float* accumulation, float* depth_median, float* depth_expected, float* scratch,
                  tn_stream_t stream);
/* its backward: tn_composite_bwd followed by tn_weights_bwd in one launch.  d_weights_in [N,S] = gradient that reaches the weights from the
 * losses (read only: the compositing term is added in registers); d_rgb [N,S,C] and d_density [N,S] are written. */
TN_API int tn_render_bwd(const float* e_bins, const float* density, const float* rgb, const float* weights, const float* d_comp,
                  const float* d_weights_in, int64_t N, int32_t S, int32_t C, float* d_rgb, float* d_density, tn_stream_t stream);

/* ---- a5..a17 in ONE call: the no-grad render of one branch (a sampler with two proposal networks + a field), i.e.
 * ThermalNerfactoModel.get_outputs at inference (models/nerfacto.py:299-353 via models/thermal_nerfacto.py:403-445; ProposalNetworkSampler
 * model_components/ray_samplers.py:577-618 without jitter; mean appearance embedding; "last_sample" background; depth clip).  The library
 * enqueues tn_spaced_bins -> tn_prop_density_fwd -> tn_weights_resample -> tn_prop_density_fwd -> tn_weights_resample ->
 * tn_field_pack_weights + tn_field_fwd -> tn_render_fwd itself: same kernels, same results as those calls made one by one.
 * nears / fars [N]; lin_spaced0 [S0+1] = linspace(0,1,S0+1), lin_pdf_k [S_k+1] = linspace(0, 1 - 1/(S_k+1), S_k+1) as the reference builds
 * them on the host; anneal = the sampler's current histogram-padding exponent.  Outputs: rgb [N,C], density [N,S2] (required);
 * accumulation, depth_median, depth_expected, prop_depth0/1 [N], e_bins_out [N,S2+1], rgb_samples_out [N,S2,C] (each may be NULL).
 * workspace: tn_render_rays_eval_workspace_bytes(N, S0, S1, S2, C) bytes, 256-byte aligned. */
TN_API int64_t tn_render_rays_eval_workspace_bytes(int64_t num_rays, int32_t S0, int32_t S1, int32_t S2, int32_t C);
TN_API int tn_render_rays_eval(const TnPropNet* prop0, const TnPropNet* prop1, const TnField* field, const float* origins,
                        const float* directions, const int64_t* camera_indices, const float* nears, const float* fars, int64_t N,
                        int32_t S0, int32_t S1, int32_t S2, float anneal, const float* lin_spaced0, const float* lin_pdf1,
                        const float* lin_pdf2, void* workspace, int64_t workspace_bytes, float* rgb, float* accumulation, float* depth_median,
                        float* depth_expected, float* prop_depth0, float* prop_depth1, float* density, float* e_bins_out,
                        float* rgb_samples_out, tn_stream_t stream);

/* The same for TRAINING: one call = CameraOptimizer.apply_to_raybundle (pose_adjustment may be NULL) + ProposalNetworkSampler with jitter
 * (jitter_k [N] or NULL per level) + Field.forward with the activations kept in field_workspace (tn_field_workspace_bytes(N*S2, 1)) for
 * tn_field_bwd + get_weights + renderers.  Launches: tn_pose_spaced_bins, tn_prop_density_fwd, tn_weights_resample, tn_prop_density_fwd,
 * tn_weights_resample, tn_field_pack_weights, tn_field_fwd(training), tn_render_fwd(training): results identical to those calls.
 * Everything later stages need goes into ONE buffer `out` (256-byte aligned); tn_render_rays_train_layout fills offsets[] (floats) with the
 * position of: 0 origins 1 directions (pose-corrected; unused when pose_adjustment is NULL) | 2 s_bins0 3 e_bins0 4 density0 5 weights0
 * 6 median0 | 7..11 the same for level 1 | 12 s_bins2 13 e_bins2 14 density2 15 weights2 | 16 rgb_samples [N,S2,C] 17 comp [N,C]
 * 18 accumulation 19 depth_median 20 depth_expected [N] | 21 scratch | 22, 23 the proposal levels' encodings, N*S0*10 and N*S1*10 floats
 * (level-major [5][N*S_k] float2; written only with save_prop_enc) | 24 = total floats; num_offsets >= TN_RENDER_TRAIN_OFFSETS.
 * save_prop_enc != 0: the proposal networks take a gradient this iteration (ray_samplers.py:591): their encodings are kept in `out`, and
 * tn_render_rays_train_bwd(prop_enc_saved != 0) reads them back instead of repeating the 40 table reads per sample -- the same values.
 * wait_event_before_field: NULL, or a hipEvent_t that `stream` waits for right before the field's first read of its parameters -- a trainer
 * that runs the previous iteration's Adam launch over the field on another stream lets it overlap the proposal sampling this way.
 * zero_fill: NULL, or zero_fill_bytes (multiple of 16) of 16-byte aligned device memory that the call clears on its way (inside the field's
 * first launch): the caller's zero-initialised accumulators of the iteration -- loss sums, d(composite), d(weights), d origins / d directions --
 * without a fill launch of their own. */
#define TN_RENDER_TRAIN_OFFSETS 25
TN_API int tn_render_rays_train_layout(int64_t num_rays, int32_t S0, int32_t S1, int32_t S2, int32_t C, int64_t* offsets, int32_t num_offsets);
TN_API int tn_render_rays_train(const TnPropNet* prop0, const TnPropNet* prop1, const TnField* field, const float* pose_adjustment,
                         const uint8_t* frozen, int32_t num_cameras, const float* origins_in, const float* directions_in,
                         const int64_t* camera_indices, const float* nears, const float* fars, int64_t N, int32_t S0, int32_t S1,
                         int32_t S2, float anneal, const float* jitter0, const float* jitter1, const float* jitter2,
                         const float* lin_spaced0, const float* lin_pdf1, const float* lin_pdf2, void* field_workspace,
                         int64_t field_workspace_bytes, float* out, void* wait_event_before_field, void* zero_fill, int64_t zero_fill_bytes,
                         int32_t save_prop_enc, tn_stream_t stream);

/* The TRAINING backward of one branch as ONE call, the counterpart of tn_render_rays_train: everything autograd runs behind d(composite) and
 * d(weights) in ThermalNerfactoModel's training step (models/thermal_nerfacto.py:403-489 backwards; cameras/rays.py:128-150,
 * model_components/renderers.py, fields/nerfacto_field.py:205-348, fields/density_fields.py:95-118 under autograd).  fwd_out is the buffer
 * tn_render_rays_train filled (same N, S, field); origins / directions [N,3] the pose-corrected rays that forward used; d_comp [N,C]; d_weights2 [N,S2] (losses on the fine weights); d_weights0 / d_weights1
 * [N,S0] / [N,S1] or both NULL when the proposal networks take no gradient this iteration (model_components/ray_samplers.py:591,605-610);
 * d_density_extra [N,S2] or NULL (the density loss's gradient on this branch's density, separate mode).  The library enqueues tn_render_bwd,
 * then -- on two companion streams of `stream` -- tn_weights_bwd + tn_prop_density_bwd per proposal level, beside tn_field_bwd on `stream`, and
 * joins: same launches and results as those calls made one by one.  tmp: tn_render_rays_train_bwd_tmp_floats(...) floats of scratch;
 * prop_workspace_k: tn_prop_workspace_bytes(N*S_k) (may be NULL without d_weights).  d_origins / d_directions [N,3] accumulate (or both NULL).
 * prop_enc_saved != 0: fwd_out holds the proposal levels' encodings (tn_render_rays_train(save_prop_enc != 0) on this buffer). */
TN_API int64_t tn_render_rays_train_bwd_tmp_floats(int64_t num_rays, int32_t S0, int32_t S1, int32_t S2, int32_t C);
TN_API int tn_render_rays_train_bwd(const TnPropNet* prop0, const TnPropNet* prop1, const TnField* field, const float* origins,
                             const float* directions, const int64_t* camera_indices, int64_t N, int32_t S0, int32_t S1, int32_t S2,
                             const float* fwd_out, const float* d_comp, const float* d_weights0,
                             const float* d_weights1, const float* d_weights2, const float* d_density_extra, void* field_workspace,
                             int64_t field_workspace_bytes, void* prop_workspace0, int64_t prop_workspace_bytes0, void* prop_workspace1,
                             int64_t prop_workspace_bytes1, float* tmp, float* d_origins, float* d_directions, int32_t prop_enc_saved,
                             tn_stream_t stream);

/* ---- a18  interlevel_loss / distortion_loss (model_components/losses.py:57-158), forward value + gradient in one pass.
 * loss_out[0] += mult * mean_over_rays(...); d_weights accumulated (may be NULL to skip the gradient). */
TN_API int tn_distortion_loss(const float* s_bins, const float* weights, int64_t N, int32_t S, float mult, float* loss_out, float* d_weights,
                       tn_stream_t stream);
TN_API int tn_interlevel_loss(const float* s_bins_fine, const float* weights_fine, int32_t S_fine, const float* s_bins_prop,
                       const float* weights_prop, int32_t S_prop, int64_t N, float mult, float* loss_out, float* d_weights_prop,
                       tn_stream_t stream);

/* Both of the above for one branch in ONE launch (the "K7" entry point of SURVEY 8b): distortion on the fine level + interlevel against each of
 * the num_props (<= TN_MAX_PROP_LEVELS) proposal levels.  s_bins_prop / weights_prop / S_prop / d_weights_prop are HOST arrays of num_props
 * entries (device pointers / sizes); d_weights_prop[i] and d_weights_fine may be NULL.  Same accumulation semantics as the single calls. */
#define TN_MAX_PROP_LEVELS 4
TN_API int tn_proposal_losses(const float* s_bins_fine, const float* weights_fine, int32_t S_fine, int32_t num_props,
                       const float* const* s_bins_prop, const float* const* weights_prop, const int32_t* S_prop,
                       float* const* d_weights_prop, int64_t N, float distortion_mult, float interlevel_mult, float* distortion_out,
                       float* interlevel_out, float* d_weights_fine, tn_stream_t stream);

/* ---- a19  ThermalNerfactoModel.get_loss_dict pixel terms (models/thermal_nerfacto.py:284-354, model_components/losses.py:602-651,
 *          utils/rgbt_utils.py:6-32): rgb MSE, thermal MSE x thermal_mult, 2x2-patch TV, cross-channel gradient loss.
 * pred_rgb [N,3], pred_thermal [N,1] (for shared mode both are views of one [N,4] buffer: pass strides in floats),
 * image [N,3], is_thermal [N] float.  losses_out[0..3] += {rgb, thermal, tv_pixel, cross_channel}; losses_out must have room for 8 floats
 * (entry 4 is scratch: the number of RGB rays); d_pred_* accumulated. */
TN_API int tn_pixel_losses(const float* pred_rgb, int32_t rgb_stride, const float* pred_thermal, int32_t thermal_stride, const float* image,
                    const float* is_thermal, int64_t N, float thermal_mult, float tv_mult, float cross_mult, float* losses_out,
                    float* d_pred_rgb, float* d_pred_thermal, tn_stream_t stream);
/* The proposal losses of one branch AND (pred_rgb != NULL) the pixel terms above in ONE launch: they are independent, and each alone is a
 * short latency-bound kernel (get_loss_dict's distortion / interlevel / rgb / thermal / tv / cross-channel terms of
 * models/thermal_nerfacto.py:284-368 side by side).  Arguments as tn_proposal_losses and tn_pixel_losses, except for where the sums go:
 * every block of every term would end with a float atomic into the same 64-byte line, and those execute one after the other (~25 ns each:
 * 40 us for 1500 blocks), so the sums are spread over loss_lines [TN_LOSS_LINES][16] (zero-filled by the caller; block b adds into line
 * b % TN_LOSS_LINES; slots 0 rgb, 1 thermal, 2 tv_pixel, 3 cross_channel, 4 / 5 ray counts per spectrum, 8 interlevel, 9 distortion) and
 * tn_losses_finish adds the lines up: losses16[k] += sum over lines of loss_lines[.][k].  tn_losses_finish also evaluates the camera
 * regulariser of one pose tensor in the same single-block launch when pose_adjustment != NULL (arguments of tn_camera_reg; reg_out may be
 * one of the 16 slots). */
#define TN_LOSS_LINES 64
TN_API int tn_train_losses(const float* s_bins_fine, const float* weights_fine, int32_t S_fine, int32_t num_props,
                    const float* const* s_bins_prop, const float* const* weights_prop, const int32_t* S_prop,
                    float* const* d_weights_prop, int64_t N, float distortion_mult, float interlevel_mult, float* d_weights_fine,
                    const float* pred_rgb, int32_t rgb_stride, const float* pred_thermal, int32_t thermal_stride, const float* image,
                    const float* is_thermal, float thermal_mult, float tv_mult, float cross_mult, float* d_pred_rgb, float* d_pred_thermal,
                    float* loss_lines, tn_stream_t stream);
/* tn_render_fwd(training) + tn_train_losses + tn_render_bwd of the shared-density model's last level in ONE launch (the renderers of
 * model_components/renderers.py:118-133,547-576, the loss terms of models/thermal_nerfacto.py:284-368 + model_components/losses.py:57-158 and the
 * renderers' backward): three wave-per-ray kernels over the same rays, each latency-bound alone.  A block renders one 2x2 patch (4 rays), hands
 * the four composites around in LDS for the pixel terms, adds the distortion term and runs the renderers' backward with the weights still in
 * registers; the interlevel terms run beside it in blocks of their own (they recompute the fine weights with the same instructions).
 * Arguments as the three entry points: C must be 4 (RGB + thermal composite; pred_rgb = comp, pred_thermal = comp + 3, d_comp [N,4] likewise),
 * N a multiple of 4; d_weights_fine [N,S] and d_comp [N,4] are accumulators (read, term added, written), d_weights_prop[i] too (or NULL);
 * d_rgb [N,S,4] and d_density [N,S] are written.  clip_depth = 0 leaves depth_expected unclipped and the per-block min / max of the sample
 * midpoints in `scratch` (tn_render_fwd's clip launch is then the caller's to issue).  Every per-element result equals the three calls' bit for
 * bit; the loss sums (loss_lines) are added up in another order, so they agree to rounding -- as two runs of tn_train_losses do. */
TN_API int tn_render_losses_bwd(const float* e_bins, const float* density, const float* rgb, int64_t N, int32_t S, int32_t C, float* weights,
                         float* comp, float* accumulation, float* depth_median, float* depth_expected, float* scratch,
                         const float* s_bins_fine, int32_t num_props, const float* const* s_bins_prop, const float* const* weights_prop,
                         const int32_t* S_prop, float* const* d_weights_prop, float distortion_mult, float interlevel_mult,
                         float* d_weights_fine, const float* image, const float* is_thermal, float thermal_mult, float tv_mult, float cross_mult,
                         float* d_comp, float* loss_lines, float* d_rgb, float* d_density, int32_t clip_depth, tn_stream_t stream);
TN_API int tn_losses_finish(const float* loss_lines, float* losses16, const float* pose_adjustment, int32_t num_cameras, float trans_pen,
                     float rot_pen, float scale, float* reg_out, float* grad_pose, tn_stream_t stream);
/* tn_pose_apply_bwd + tn_losses_finish for the same pose tensor in one launch (the end of an iteration's backward); loss_lines / losses16 may
 * both be NULL (regulariser only). */
TN_API int tn_pose_bwd_finish(const float* pose_adjustment, const uint8_t* frozen, const int64_t* camera_indices, const float* directions_in,
                       const float* d_origins, const float* d_directions, int64_t N, int32_t num_cameras, float* grad_pose,
                       const float* loss_lines, float* losses16, float trans_pen, float rot_pen, float scale, float* reg_out,
                       tn_stream_t stream);
/* tn_pose_bwd_finish + GradScaler's non-finite check of what the table scatters do not see, in the same launch: found_inf[pose_flag] is raised
 * when a contribution to the pose gradient is inf / NaN, and found_inf[flag_index[k]] when any of the `counts[k]` gradients at grads + offsets[k]
 * is (up to 8 SMALL ranges -- MLP weights, embeddings: at most 4 M floats each; offsets / counts / flag_index are HOST arrays).  With
 * TnGrid::nonfinite_flag on every grid this replaces tn_grad_nonfinite_ranges over the whole gradient arena. */
TN_API int tn_pose_bwd_finish_check(const float* pose_adjustment, const uint8_t* frozen, const int64_t* camera_indices, const float* directions_in,
                             const float* d_origins, const float* d_directions, int64_t N, int32_t num_cameras, float* grad_pose,
                             const float* loss_lines, float* losses16, float trans_pen, float rot_pen, float scale, float* reg_out,
                             const float* grads, int32_t num_ranges, const int64_t* offsets, const int64_t* counts, const int32_t* flag_index,
                             int32_t num_flags, float* found_inf, int32_t pose_flag, tn_stream_t stream);
/* density L1 cross loss with the reference's detach asymmetry (models/thermal_nerfacto.py:328-344): loss += a*mean|x-y| with
 * gradient weight gx to x and gy to y (accumulated; either may be NULL). */
TN_API int tn_l1_loss(const float* x, const float* y, int64_t count, float gx, float gy, float* loss_out, float* d_x, float* d_y,
               tn_stream_t stream);
/* per-iteration metrics in one launch (models/thermal_nerfacto.py:262-270 PSNR per spectrum from the tn_pixel_losses sums losses[0,1,4,5];
 * cameras/camera_optimizers.py:197-202 pose norms): metrics_out[0] psnr_rgb, [1] psnr_thermal, [2],[3] |pose0[:, :3]|, |pose0[:, 3:]|,
 * [4],[5] the same for pose1; either pose may be NULL. */
TN_API int tn_train_metrics(const float* losses, int64_t N, float thermal_mult, const float* pose0, int32_t num_cameras0, const float* pose1,
                     int32_t num_cameras1, float* metrics_out, tn_stream_t stream);
/* camera regulariser (cameras/camera_optimizers.py:189-195). */
TN_API int tn_camera_reg(const float* pose_adjustment, int32_t num_cameras, float trans_pen, float rot_pen, float scale, float* loss_out,
                  float* grad_pose, tn_stream_t stream);

/* ---- N1  torch.optim.Adam(lr, eps) as engine/optimizers.py:73-210 builds it, fused over a flat fp32 arena.
 * step is 1-based. */
TN_API int tn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count, int32_t step, double lr,
                 double beta1, double beta2, double eps, tn_stream_t stream);
/* The same for several ranges of one set of arenas in ONE launch: range k covers elements [offsets[k], offsets[k] + counts[k]) (offsets
 * multiples of 4) with its own 1-based step count and learning rate -- the optimiser groups of engine/optimizers.py:86-112.  offsets, counts,
 * steps, lrs are HOST arrays of num_ranges (<= 8) entries. */
TN_API int tn_adam_step_ranges(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t num_ranges, const int64_t* offsets,
                        const int64_t* counts, const int32_t* steps, const double* lrs, double beta1, double beta2, double eps,
                        tn_stream_t stream);
/* GradScaler semantics without a host round trip (engine/trainer.py:470-495 -> torch/amp/grad_scaler.py; engine/optimizers.py:144-183).
 * GradScaler decides per optimiser, i.e. per parameter group: found_inf is a device array of num_flags floats, one per group.
 *  - tn_grad_nonfinite sets *found_inf = 1 when any of `count` gradients is inf or NaN (it never clears it: zero-fill once per step).
 *  - tn_adam_step_ranges_amp is tn_adam_step_ranges with the decision on the device.  Range k belongs to group flag_index[k] (HOST array, NULL =
 *    all 0):  found_inf[flag] != 0 -> range k is not touched (parameters and both moments bit-identical) and, when count_skip != 0,
 *    skipped[flag] += 1 (once per flag and launch, however many ranges carry it);  inv_scale (device float or NULL): gradients are multiplied by *inv_scale as they are read;  skipped (device int32
 *    array or NULL): the bias corrections use steps[k] - skipped[flag], as torch's fused Adam keeps its step tensors (torch/optim/adam.py:
 *    step -= found_inf);  lr_finals / sched_max_steps (HOST arrays or NULL) + sched_step: when given, lrs[k] is lr_init and the kernel
 *    evaluates the reference's ExponentialDecayScheduler (engine/schedulers.py:109-141) at sched_step - skipped[lag_index] (lag_index = -1:
 *    no lag): the trainer does not step the schedulers in an iteration whose scale dropped (engine/trainer.py:491-495).
 *    zero_grads != 0: the launch CONSUMES the gradients of its ranges -- sets them to zero behind the read, also when the step is skipped --
 *    (`grads` is then written): the optimizers.zero_grad_some() of the next iteration (engine/trainer.py:463-467) without a fill launch.
 *  - tn_grad_scaler_update is GradScaler.update() on the device (backoff / growth of *scale, growth tracker) and adds 1 to *lag (may be NULL)
 *    when any of the num_flags entries of found_inf is set; clear_found_inf != 0 zero-fills found_inf afterwards (ready for the next step). */
TN_API int tn_grad_nonfinite(const float* grads, int64_t count, float* found_inf, tn_stream_t stream);
/* the same for up to 8 ranges of one gradient arena in ONE launch: range k raises found_inf[flag_index[k]] (offsets, counts, flag_index: HOST arrays) */
TN_API int tn_grad_nonfinite_ranges(const float* grads, int32_t num_ranges, const int64_t* offsets, const int64_t* counts, const int32_t* flag_index,
                             int32_t num_flags, float* found_inf, tn_stream_t stream);
TN_API int tn_adam_step_ranges_amp(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t num_ranges, const int64_t* offsets,
                            const int64_t* counts, const int32_t* steps, const double* lrs, const double* lr_finals,
                            const int32_t* sched_max_steps, int32_t sched_step, double beta1, double beta2, double eps,
                            const float* inv_scale, const float* found_inf, const int32_t* flag_index, int32_t num_flags, int32_t* skipped,
                            int32_t lag_index, int32_t count_skip, int32_t zero_grads, tn_stream_t stream);
TN_API int tn_grad_scaler_update(float* scale, int32_t* growth_tracker, float* found_inf, int32_t num_flags, int32_t* lag,
                          double growth_factor, double backoff_factor, int32_t growth_interval, int32_t clear_found_inf, tn_stream_t stream);
/* tn_adam_step_ranges_amp + tn_grad_scaler_update(clear_found_inf = 1) in ONE launch: the last block of the Adam launch to finish performs
 * GradScaler.update() -- every block has read found_inf / the schedule lag by then.  done_counter: TN_ADAM_DONE_WORDS zeroed uint32 on the device
 * (left zero; the blocks count themselves in on 64 counters in 64 different 64-byte lines: same-line atomics execute one after the other). */
#define TN_ADAM_DONE_WORDS (65 * 16)
TN_API int tn_adam_step_ranges_amp_update(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t num_ranges, const int64_t* offsets,
                                   const int64_t* counts, const int32_t* steps, const double* lrs, const double* lr_finals,
                                   const int32_t* sched_max_steps, int32_t sched_step, double beta1, double beta2, double eps,
                                   const float* inv_scale, float* found_inf, const int32_t* flag_index, int32_t num_flags, int32_t* skipped,
                                   int32_t lag_index, int32_t count_skip, int32_t zero_grads, float* scale, int32_t* growth_tracker,
                                   uint32_t* done_counter, double growth_factor, double backoff_factor, int32_t growth_interval,
                                   tn_stream_t stream);
TN_API int tn_fill_zero(void* ptr, int64_t bytes, tn_stream_t stream);

/* ---- Trainer.train_iteration (engine/trainer.py:455-499) for the shared-density model with a camera optimiser, as ONE call: what
 * RenderEngine.train_step enqueues through five calls of this ABI, in the same order on the same streams --
 *   tn_render_rays_train      forward of the branch (pose correction, proposal sampling, field, renderers); the accumulators in `acc` are cleared
 *                             inside the field's first launch
 *   tn_train_losses           pixel terms + distortion + both interlevel terms (value and gradient), sums spread over loss_lines
 *   tn_render_rays_train_bwd  renderer backward, field backward (d position, table scatter), both proposal networks when prop_grad != 0
 *                             (with TN_FUSE_RENDER=1 the renderers at the end of the first, the losses and the renderer backward at the head of the
 *                             third are ONE launch, tn_render_losses_bwd: every gradient and output bit for bit either way, the loss sums to
 *                             rounding)
 *   tn_pose_bwd_finish_check  pose gradient + camera regulariser + loss sums into losses16, GradScaler's found_inf for the pose and the small
 *                             ranges no table scatter sees
 *   tn_adam_step_ranges_amp_update   Adam over the stepped groups (skip / bias correction / LR schedule decided on the device), GradScaler.update()
 * A host that drives training through this entry point spends one call (~0.11 ms of launch time) per iteration; through the Python binding the
 * host side of an iteration drops from 0.39 to 0.22 ms (scripts/trace_fused_host.py, 1024 rays).  The iteration itself is GPU-bound at either
 * batch size (0.44 ms at 1024 rays, 0.83 ms at 4096): the wall time does not change, the host thread is free for the other 0.2 ms.
 * Every pointer is a device pointer unless it says HOST; buffers as the five entry points document them.
 * `acc` (acc_bytes, 16-byte aligned, multiple of 16): ONE allocation holding losses16 [16], loss_lines [TN_LOSS_LINES][16], d_comp [N,C],
 * d_weights2 [N,S2], d_weights0 [N,S0], d_weights1 [N,S1] (both only read when prop_grad != 0), d_origins, d_directions [N,3]; the call clears it. */
#define TN_TRAIN_STEP_MAX_RANGES 8
/* The NEXT iteration's sampling front -- everything tn_render_rays_train runs before the field: CameraOptimizer.apply_to_raybundle
 * (cameras/camera_optimizers.py:130-176), the level-0 bins and twice density_fn -> get_weights -> PDFSampler (model_components/ray_samplers.py:577-618)
 * -- for the batch TnTrainStep::next_sample describes, as co-work of THIS iteration's optimiser launch: five short launches (86 us at 4096 rays) that
 * are bound by instruction issue leave the head of every iteration and run beside the Adam pass over the field, which is bound by HBM and touches
 * none of their inputs.  One wave takes one ray through the whole chain (no ray depends on another); the optimiser groups the chain READS (the
 * proposal networks, the pose corrections: whatever range of `params` holds prop0 / prop1 / pose_adjustment) are stepped by a launch of their own
 * in front, so it sees this iteration's final parameters.  Results land in fwd_out exactly where tn_render_rays_train puts them (origins ... e_bins2,
 * and the proposal encodings when prop_grad != 0), bit for bit.  Uses this call's nears / fars / lin_* tables / pose / frozen / networks and N rays.
 * Taken only when next_sample is, next_sample->num_rays == N, 128 < S0 <= 256, 64 < S1 <= 128 (the sampler's default lane layouts) and at least one
 * stepped range is not read by the chain. */
typedef struct TnNextSampling {
  float* fwd_out;                                                   /* the NEXT iteration's forward buffer (same layout: same N, S0, S1, S2) */
  const float* jitter0; const float* jitter1; const float* jitter2; /* the NEXT iteration's jitter [N] (or NULL) */
  float anneal;                                                     /* the NEXT iteration's histogram-padding exponent */
  int32_t prop_grad;                                                /* the NEXT iteration's prop_grad: != 0 keeps the proposal encodings */
} TnNextSampling;
typedef struct TnTrainStep {
  const TnPropNet* prop0; const TnPropNet* prop1; const TnField* field;  /* HOST structs, gradient pointers set */
  /* the iteration's batch (datamanager.next_train): rays before the pose correction, ground truth */
  const float* origins_in; const float* directions_in; const int64_t* camera_indices; const float* image; const float* is_thermal;
  const float* nears; const float* fars;
  int64_t N; int32_t S0, S1, S2;
  /* camera optimiser */
  const float* pose_adjustment; const uint8_t* frozen; int32_t num_cameras; float* grad_pose;
  float trans_pen, rot_pen, pen_scale;
  /* sampler */
  float anneal; int32_t prop_grad;
  const float* jitter0; const float* jitter1; const float* jitter2; const float* lin_spaced0; const float* lin_pdf1; const float* lin_pdf2;
  /* buffers */
  void* field_workspace; int64_t field_workspace_bytes;
  void* prop_workspace0; int64_t prop_workspace_bytes0; void* prop_workspace1; int64_t prop_workspace_bytes1;
  float* fwd_out;   /* tn_render_rays_train_layout: offsets[TN_RENDER_TRAIN_OFFSETS - 1] floats, 256-byte aligned */
  float* bwd_tmp;   /* tn_render_rays_train_bwd_tmp_floats */
  void* acc; int64_t acc_bytes;
  float* losses16; float* loss_lines; float* d_comp; float* d_weights0; float* d_weights1; float* d_weights2; float* d_origins; float* d_directions;
  /* loss multipliers (models/thermal_nerfacto.py:32-64, models/nerfacto.py:52-133) */
  float thermal_mult, tv_mult, cross_mult, distortion_mult, interlevel_mult;
  /* GradScaler's check of the small gradient ranges (tn_pose_bwd_finish_check) */
  int32_t num_check; int64_t check_offsets[TN_TRAIN_STEP_MAX_RANGES]; int64_t check_counts[TN_TRAIN_STEP_MAX_RANGES];
  int32_t check_flags[TN_TRAIN_STEP_MAX_RANGES]; int32_t pose_flag;
  /* Adam + GradScaler.update (tn_adam_step_ranges_amp_update); num_ranges == 0: no optimiser launch */
  float* params; float* grads; float* exp_avg; float* exp_avg_sq;
  int32_t num_ranges; int64_t offsets[TN_TRAIN_STEP_MAX_RANGES]; int64_t counts[TN_TRAIN_STEP_MAX_RANGES]; int32_t steps[TN_TRAIN_STEP_MAX_RANGES];
  double lrs[TN_TRAIN_STEP_MAX_RANGES]; double lr_finals[TN_TRAIN_STEP_MAX_RANGES]; int32_t sched_max_steps[TN_TRAIN_STEP_MAX_RANGES];
  int32_t flag_index[TN_TRAIN_STEP_MAX_RANGES]; int32_t sched_step;
  double beta1, beta2, eps;
  float* found_inf; int32_t num_flags; int32_t* skipped; int32_t lag_index;
  float* scale; int32_t* growth_tracker; uint32_t* done_counter; double growth_factor, backoff_factor; int32_t growth_interval;
  /* NULL, or the NEXT iteration's batch (HOST struct): sampled in co-work blocks of the optimiser launch; ignored (the caller's to launch,
   * tn_sample_rays_args) when num_ranges == 0 -- *next_sample_taken (HOST, may be NULL) says which */
  const TnSampleRays* next_sample; int32_t* next_sample_taken;
  /* NULL, or (with next_sample) the NEXT iteration's sampling front (HOST struct, see TnNextSampling): run for that batch in the same co-work blocks.
   * *next_sampling_taken (HOST, may be NULL) = 1 when the optimiser launch carried it: the next call then passes sampling_done = 1. */
  const struct TnNextSampling* next_sampling; int32_t* next_sampling_taken;
  /* != 0: the previous call's next_sampling has filled fwd_out up to the field's bins for THIS batch (origins_in / directions_in / camera_indices are
   * next_sample's outputs), with this call's jitter, anneal and prop_grad, and no parameter of the proposal networks or the poses has changed
   * since: the forward starts at the field. */
  int32_t sampling_done;
} TnTrainStep;
TN_API int tn_train_step(const TnTrainStep* step, tn_stream_t stream);
/* ---- 8e  the data-parallel gradient exchange for a host that binds only this ABI: what torch DDP does for the reference
 * (pipelines/base_pipeline.py:281-283: mean all-reduce of the gradients over NCCL; scripts/train.py:138-151 starts one process per GPU).
 * RCCL is resolved at the first call -- from the RCCL the process has loaded already (PyTorch's own), else librccl.so on the loader path -- and is
 * not a link-time dependency of the library; without one these calls return TN_ELAUNCH.  (The Python package exchanges through torch.distributed,
 * nerfstudio_thermal_amd/parallel.py: the same library underneath.)
 *   tn_comm_unique_id(out)            rank 0: 128 bytes (HOST) to hand to every rank (ncclGetUniqueId)
 *   tn_comm_create(id, world, rank, &comm)   every rank, collectively, on its CURRENT device (ncclCommInitRank)
 *   tn_allreduce_grads(comm, grads, count, average, stream)   in place over `count` floats of the caller's gradient arena, enqueued on `stream`:
 *                                     average != 0 -> the mean over the ranks (ncclAvg), else the sum.  Any slice of the arena, as often as the
 *                                     caller's schedule wants (the whole live range behind the backward, or level ranges behind their folds).
 *   tn_comm_destroy(comm) */
TN_API int tn_comm_unique_id(void* unique_id_out);
TN_API int tn_comm_create(const void* unique_id, int32_t world_size, int32_t rank, void** comm_out);
TN_API int tn_comm_destroy(void* comm);
TN_API int tn_allreduce_grads(void* comm, float* grads, int64_t count, int32_t average, tn_stream_t stream);

/* waits for and destroys the library's companion streams (see "State and environment" at the top); 0 or TN_ELAUNCH */
TN_API int tn_shutdown(void);

/* ---------------------------------------------------------------------------------------------------------------------------
 * N4: forward Gaussian-splat render, RGB + thermal colour per Gaussian.  Replaces the gsplat calls of
 * SplatfactoModel.get_outputs (nerfstudio/models/splatfacto.py:739-807): project_gaussians, spherical_harmonics, rasterize_gaussians
 * (colour and depth).  gsplat is a third-party package outside the reference tree: parity is UNPINNED (oracle/splat_oracle.py restates
 * its published algorithm).  16x16 tiles (splatfacto.py:738). */
typedef struct TnSplatCamera {
  float viewmat[12];  /* world -> camera, rows of the 3x4 matrix in gsplat's convention (x right, y down, z forward): splatfacto.py:700-712 */
  float projmat[16];  /* projection_matrix(0.001, 1000, fovx, fovy) @ viewmat, row-major 4x4: splatfacto.py:718,745 */
  float fx, fy, cx, cy;
  float position[3];  /* camera centre in world space (view directions of the SH colours, splatfacto.py:770) */
  float clip_thresh;  /* near clip in view space (gsplat default 0.01) */
  int32_t width, height;
} TnSplatCamera;
/* scratch for num_gaussians Gaussians and up to max_intersections (Gaussian, tile) pairs; num_tiles = ceil(W/16) * ceil(H/16) */
TN_API int64_t tn_splat_workspace_bytes(int64_t num_gaussians, int64_t max_intersections, int32_t num_tiles);
/* project_gaussians + spherical_harmonics (splatfacto.py:739-777).  means [N,3], log_scales [N,3] (exponentiated inside), quats [N,4]
 * (w,x,y,z; normalised inside), opacities [N] (logits), features_dc [N,3], features_rest [N,K,3], thermal_dc [N,1], thermal_rest [N,K,1]
 * (K = num_rest_coeffs).  sh_degree 0..3 = degree evaluated this step (min(step // interval, sh_degree)); -1 = sigmoid(features_dc)
 * (config.sh_degree == 0).  antialiased != 0: opacity x compensation (rasterize_mode "antialiased").  Outputs as gsplat returns them:
 * xys [N,2], depths [N], radii [N] int32, conics [N,3], compensation [N], num_tiles_hit [N] int32, plus tile_box [N,4] int32
 * (x0, y0, x1, y1 in tiles).  Colours and opacities go into the workspace for tn_splat_raster.
 *
 * Optional inputs of the splat entry points are GROUPS of nullable pointers: a group is given whole or not at all, and a partly given group is
 * TN_EINVAL before any launch.  Which groups a call gives picks the instantiation of the same kernel.  Here, each on its own:
 *   pose_camera        the record tn_splat_pose_camera wrote (DEVICE): view, projection rows and position come from it (camera still gives the
 *                      intrinsics, the clip threshold and the image size).
 *   opacities_thermal  [N] logits: separate thermal opacity (see "N4 separate thermal opacity" below); max_intersections must then be >= 0.
 *   crop               a TnSplatCrop (HOST, read before the launch; see "N4 crop box" below): the box test on the mean comes first; a Gaussian
 *                      outside leaves exactly as one behind the clip plane does (radius 0, no tiles, zeros in every output), one inside goes
 *                      through the same arithmetic as without the box, and a block whose Gaussians are all outside does not read its higher-order
 *                      SH coefficients.  tn_splat_bin and the rasters run unchanged on what this leaves: the frame of the Gaussians inside, bit for
 *                      bit. */
typedef struct TnSplatCrop TnSplatCrop;
TN_API int tn_splat_project(const TnSplatCamera* camera, const float* pose_camera, const float* means, const float* log_scales, const float* quats,
                            const float* opacities, const float* features_dc, const float* features_rest, const float* thermal_dc,
                            const float* thermal_rest, const float* opacities_thermal, int64_t num_gaussians, int32_t num_rest_coeffs,
                            int32_t sh_degree, int32_t antialiased, float* xys, float* depths, int32_t* radii, float* conics, float* compensation,
                            int32_t* num_tiles_hit, int32_t* tile_box, void* workspace, int64_t max_intersections, const TnSplatCrop* crop,
                            tn_stream_t stream);
/* tile binning of rasterize_gaussians: depth sort of the Gaussians, scan, (tile, Gaussian) pairs in depth order, stable radix sort by
 * tile, tile ranges.  The pairs come from the TIGHT tile boxes tn_splat_project left in the workspace (gsplat's 3-sigma box cut down to
 * the tiles where alpha >= 1/255 is reachable: exact, fewer pairs than sum(num_tiles_hit)).  Reads the pair count back to the host
 * (*num_intersections_out, a HOST pointer; one stream synchronisation, as gsplat's binning does); returns TN_EINVAL with the needed count
 * in *num_intersections_out when it exceeds max_intersections. */
TN_API int tn_splat_bin(const TnSplatCamera* camera, const float* depths, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                 int64_t* num_intersections_out, tn_stream_t stream);
/* rasterize_gaussians, colour (RGB + thermal over background4) and depth in one pass (splatfacto.py:789-809): out_rgbt [H,W,4] clamped to
 * <= 1, out_depth [H,W] = depth / alpha where alpha > 0, else the maximum of the un-normalised depth image, out_alpha [H,W]. */
TN_API int tn_splat_raster(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections, const float* background4,
                    int32_t antialiased, float* out_rgbt, float* out_depth, float* out_alpha, tn_stream_t stream);

/* tn_splat_raster with every optional output.  Groups:
 *   {out_alpha_thermal}                              [H,W], the thermal chain's accumulation, on a frame projected with opacities_thermal
 *                                                    (out_rgbt's thermal channel then comes from that chain, out_alpha is the RGB chain's);
 *   {out_transmittance, out_last}                    the training render: per pixel the final T [H,W] and, int32 [H,W], the number of entries of
 *                                                    the pixel's tile list up to and including the last Gaussian that contributed (0 = none).
 *                                                    out_rgbt then holds the colour BEFORE the clamp to 1 (the caller clamps, and owns the clamp's
 *                                                    gradient);
 *   {out_transmittance_thermal, out_last_thermal}    the same of the thermal chain; given exactly when both groups above are.
 * out_depth and out_alpha are as tn_splat_raster writes them.  Refuses null pointers and negative sizes. */
TN_API int tn_splat_raster_chains(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                  const float* background4, int32_t antialiased, float* out_rgbt, float* out_depth, float* out_alpha,
                                  float* out_alpha_thermal, float* out_transmittance, int32_t* out_last, float* out_transmittance_thermal,
                                  int32_t* out_last_thermal, tn_stream_t stream);

/* ---- N4 backward: the exact derivative of the render above with respect to the Gaussians (rgb, thermal, accumulation; depth with the depth
 * group).  Deterministic: no float atomics, the same inputs give bit-identical gradients.  Call order of one training frame:
 * tn_splat_project -> tn_splat_bin -> tn_splat_raster_chains, then tn_splat_raster_backward -> tn_splat_project_backward on the SAME
 * workspace (nothing may run a frame through it in between), with the same groups throughout.
 *
 * scratch of tn_splat_raster_backward: one record of partial gradients per (Gaussian, tile) pair -- one more sum with the thermal chain (sep), two
 * more with v_xys_abs (absgrad), one more with the depth group (depth); each flag 0 or 1 -- and a per-Gaussian map; -1 on bad sizes */
TN_API int64_t tn_splat_backward_workspace_bytes(int64_t num_gaussians, int64_t max_intersections, int32_t sep, int32_t absgrad, int32_t depth);
/* raster backward.  num_intersections = tn_splat_bin's count; antialiased = the frame's flag; transmittance / last from tn_splat_raster_chains;
 * conics [N,3] from tn_splat_project; v_rgbt [H,W,4] = dL / d(colour before the clamp), v_alpha [H,W] = dL / d accumulation.  Outputs per Gaussian:
 * v_xys [N,2], v_conics [N,3], v_colors [N,4] (RGB + thermal after the SH clamp / sigmoid), v_log_opacity [N] = dL / d ln(opacity used by the
 * rasteriser, x compensation in antialiased mode).  Gaussians the forward culled get zeros.  Groups:
 *   {transmittance_thermal, last_thermal, v_alpha_thermal, v_log_opacity_thermal}   both chains: v_rgbt's RGB channels and v_alpha feed the RGB
 *       chain, its thermal channel and v_alpha_thermal [H,W] the thermal chain; v_xys and v_conics are the sums over both; v_log_opacity_thermal [N]
 *       = dL / d ln(the thermal opacity as the rasteriser used it).
 *   {v_xys_abs}   absgrad (AbsGS; gsplat's `absgrad`, splatfacto's `use_absgrad`): [N,2] = sum over the pixels p a Gaussian blends of (|J_p.x|,
 *       |J_p.y|), where J_p = d sigma_p * (cx dx + cy dy, cy dx + cz dy) is the pixel's term of v_xys (with both chains d sigma_p is the sum of both
 *       chains' terms, taken before the absolute value).  A blend on the 0.999 clamp contributes nothing, a Gaussian without a pair gets (0, 0).
 *       Nothing is chained through it, so the projection backward is unchanged.
 *   {depth, v_depth, v_depths}   the depth gradient (see "N4 depth gradient" below): depth [H,W] = the normalised image the forward wrote, v_depth
 *       [H,W] = dL / d depth, v_depths [N] = dL / d depths (out).  Refused with antialiased != 0.
 * Every output a group does not add is bit-equal with and without it.  Refuses a bad Gaussian count, num_intersections outside
 * [0, max_intersections], null pointers (N > 0) and a bwd_workspace_bytes below tn_splat_backward_workspace_bytes of the groups given. */
TN_API int tn_splat_raster_backward(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                    int64_t num_intersections, const float* background4, int32_t antialiased, const float* transmittance,
                                    const int32_t* last, const float* transmittance_thermal, const int32_t* last_thermal, const float* conics,
                                    const float* v_rgbt, const float* v_alpha, const float* v_alpha_thermal, void* bwd_workspace,
                                    int64_t bwd_workspace_bytes, float* v_xys, float* v_xys_abs, float* v_conics, float* v_colors,
                                    float* v_log_opacity, float* v_log_opacity_thermal, const float* depth, const float* v_depth, float* v_depths,
                                    tn_stream_t stream);
/* projection + SH backward: the parameters and settings of the tn_splat_project call, its radii, and tn_splat_raster_backward's outputs ->
 * gradients in the parameters' layouts: v_means [N,3], v_log_scales [N,3], v_quats [N,4] (through the normalisation), v_opacities [N]
 * (logits), v_features_dc [N,3], v_features_rest [N,K,3], v_thermal_dc [N,1], v_thermal_rest [N,K,1] (zero beyond sh_degree).  The view
 * directions of the SH colours carry no gradient (splatfacto.py:770 detaches the means there).  Groups:
 *   {opacities_thermal, v_log_opacity_thermal, v_opacities_thermal}   v_opacities_thermal [N] (logits) from v_log_opacity_thermal; in antialiased
 *       mode the covariance receives the compensation's gradient from both opacities.
 *   {pose_camera, pose_row, workspace, grad_pose_row}   for a frame projected with pose_camera (the same record, and the row it was made from): the
 *       pose gradient.  Every Gaussian with radii > 0 contributes to dL/d view' through its view-space point (frustum clamp included), the
 *       covariance's T = J W and the projection rows xys reads; the 12 sums are reduced per wave, per block (double) and over the blocks in block
 *       order -- no float atomics, bit-reproducible -- and chained through D to the row.  The result is ADDED to grad_pose_row [6] (the caller's row
 *       of a zeroed or accumulating grad_pose [C,6]); dview_out [12] (optional inside the group) receives dL/d view'.  workspace:
 *       tn_splat_pose_workspace_bytes; workspace_bytes is ignored without the group.
 *   {v_depths}   [N] = dL / d depths, what the raster backward's depth group left: depths[i] is the view-space z of the mean, so every Gaussian with
 *       radii > 0 adds v_depths[i] * view[2, :3] to v_means, and with a pose v_depths[i] * (mean, 1) to row 2 of dL/d view' before the
 *       double-precision sums.  Refused with antialiased != 0. */
TN_API int tn_splat_project_backward(const TnSplatCamera* camera, const float* pose_camera, const float* pose_row, const float* means,
                                     const float* log_scales, const float* quats, const float* opacities, const float* features_dc,
                                     const float* features_rest, const float* thermal_dc, const float* thermal_rest, const float* opacities_thermal,
                                     int64_t num_gaussians, int32_t num_rest_coeffs, int32_t sh_degree, int32_t antialiased, const int32_t* radii,
                                     const float* v_xys, const float* v_conics, const float* v_colors, const float* v_log_opacity,
                                     const float* v_log_opacity_thermal, const float* v_depths, float* v_means, float* v_log_scales, float* v_quats,
                                     float* v_opacities, float* v_features_dc, float* v_features_rest, float* v_thermal_dc, float* v_thermal_rest,
                                     float* v_opacities_thermal, void* workspace, int64_t workspace_bytes, float* grad_pose_row, float* dview_out,
                                     tn_stream_t stream);

/* ---- N4 refinement: splatfacto's densification, culling and statistics (SplatfactoModel.after_train / refinement_after,
 * nerfstudio/models/splatfacto.py:346-498).  No float atomics: the results are bit-reproducible.
 * The thresholds of SplatfactoModelConfig (splatfacto.py:103-172) and what the decisions read besides them.  The step rules are the
 * reference's: densify iff step < stop_split_at and step % (reset_alpha_every * refine_every) > num_train_data + refine_every; otherwise cull
 * only iff step >= stop_split_at and continue_cull_post_densification; huge-Gaussian culls iff step > refine_every * reset_alpha_every;
 * screen-size splits and culls iff step < stop_screen_size_at. */
typedef struct TnSplatRefine {
  float cull_alpha_thresh;
  float cull_scale_thresh;
  float densify_grad_thresh;
  float densify_size_thresh;
  float cull_screen_size;
  float split_screen_size;
  int32_t refine_every;
  int32_t reset_alpha_every;
  int32_t stop_screen_size_at;
  int32_t stop_split_at;
  int32_t n_split_samples;                  /* 1..16 */
  int32_t continue_cull_post_densification;
  int32_t num_train_data;
  int32_t max_size;                         /* max(H, W) of the last training frame (the reference's last_size) */
} TnSplatRefine;
/* after_train's statistics for one training frame: xys_grad [N,2] = dL / d xys, radii [N] of that frame, max_size = its max(H, W).
 * first != 0 (the first call after a reset): grad_norm_sum = |xys_grad|, vis_counts = 1 for every Gaussian and max_2d_size starts at 0;
 * otherwise only visible Gaussians (radii > 0) add |xys_grad| and 1.  Visible Gaussians then take max_2d_size = max(max_2d_size, radii / max_size). */
TN_API int tn_splat_grad_stats(const float* xys_grad, const int32_t* radii, int64_t num_gaussians, int32_t max_size, int32_t first,
                               float* grad_norm_sum, float* vis_counts, float* max_2d_size, tn_stream_t stream);
/* scratch of tn_splat_refine_plan / tn_splat_refine_apply (worst case: every Gaussian split and duplicated); -1 on bad sizes */
TN_API int64_t tn_splat_refine_workspace_bytes(int64_t num_gaussians, int32_t n_split_samples);
/* Classifies every Gaussian (split, duplicate, cull of each row it ends up in) and places every surviving output row.  counts_out (HOST,
 * 4 entries): split Gaussians, surviving originals, surviving split children (all samples), surviving duplicates.  One device-to-host copy
 * of the counts (a stream synchronisation).  When the step neither densifies nor culls nothing is launched and the counts are (0, N, 0, 0).
 * With opacities_thermal [N] (optional) the both-below cull rule: a Gaussian is culled for low opacity only when sigmoid(opacities) AND
 * sigmoid(opacities_thermal) are below cull_alpha_thresh (one that is visible in either spectrum stays). */
TN_API int tn_splat_refine_plan(const TnSplatRefine* config, int32_t step, const float* log_scales, const float* opacities,
                                const float* opacities_thermal, const float* grad_norm_sum, const float* vis_counts, const float* max_2d_size,
                                int64_t num_gaussians, void* workspace, int64_t workspace_bytes, int64_t* counts_out, tn_stream_t stream);
/* Writes the refined Gaussians: rows = surviving originals, split children (sample-major, in index order), duplicates (in index order).
 * params / exp_avg / exp_avg_sq / new_*: HOST arrays of num_tensors device pointers (8 or 9; anything else is refused) in the order means [N,3],
 * log-scales [N,3], quats [N,4], opacities [N,1], features_dc [N,3], features_rest [N,K,3], features_dc_thermal [N,1], features_rest_thermal
 * [N,K,1] (K = num_rest_coeffs; the two rest entries are ignored when K = 0) and, ninth, opacities_thermal [N,1], which -- with its moments -- is
 * carried exactly as the opacities are.  A parameter's four moment pointers are all null (no Adam state) or all set.  Outputs hold
 * counts[1] + counts[2] + counts[3] rows.  Surviving originals keep their moments, new rows get zero moments.  Split children take
 * mean + R(q / |q|) (exp(log-scale) * noise row) and log(exp(log-scale) / 1.6); noise [counts[0] * n_split_samples, 3] is torch.randn's sample-major
 * layout.  counts and workspace must be those of the tn_splat_refine_plan call on the same inputs. */
TN_API int tn_splat_refine_apply(const TnSplatRefine* config, int64_t num_gaussians, int32_t num_rest_coeffs, const void* workspace,
                                 int64_t workspace_bytes, const int64_t* counts, const float* noise, int32_t num_tensors, const float* const* params,
                                 const float* const* exp_avg, const float* const* exp_avg_sq, float* const* new_params, float* const* new_exp_avg,
                                 float* const* new_exp_avg_sq, tn_stream_t stream);

/* ---- N4 separate thermal opacity (ThermalSplatfactoModelConfig.thermal_opacity_mode = "separate", the splat analogue of thermal-nerfacto's
 * density_mode "separate"): every Gaussian has a second opacity logit, opacities_thermal [N].  RGB, accumulation and depth composite with
 * sigmoid(opacities) as above; the thermal channel composites with sigmoid(opacities_thermal) through a transmittance chain of its own over the
 * same depth-sorted tile lists, with its own stop (a pixel's chain stops before the Gaussian that would take T to 1e-4 or below), and the thermal
 * background is weighted by that chain's final transmittance.  In antialiased mode both opacities take the same compensation.  It is the thermal
 * group of every entry point above, and a frame gives it throughout or not at all (a workspace projected without opacities_thermal holds no
 * thermal opacities).  In the projection the tight tile box and the half extents of {alpha >= 1/255} come from the LARGER of the two opacities, so
 * neither chain loses a contributor; radii, num_tiles_hit and tile_box are gsplat's, as before.  Same determinism: no float atomics, bit-identical
 * gradients for the same inputs. */
/* ThermalNeRF's removal renders (models/thermal_nerfacto.py:460-487, with opacities for densities): the frame composited only from the
 * Gaussians on which the two spectra agree.  One more launch over the tile lists of a frame, after tn_splat_project (with opacities_thermal) and tn_splat_bin on the
 * same workspace (before or after tn_splat_raster_chains; it reads the workspace only).  With o = sigmoid(opacities), ot = sigmoid(opacities_thermal)
 * and thr = min_opacity_diff: out_removal [H,W,4] holds in .xyz the RGB colour composited as tn_splat_raster_chains' RGB chain does, except that a
 * Gaussian with |o - ot| < thr * o false has alpha 0, over background4.xyz with this chain's own final transmittance; in .w the thermal colour
 * likewise with ot's chain, |ot - o| < thr * ot, and background4.w; both clamped to <= 1.  The comparisons are strict and use the plain
 * opacities (in antialiased mode the chains blend with the compensated ones, as the workspace holds them): thr = 0 keeps nothing -- the
 * background --, thr = inf everything -- tn_splat_raster_chains' out_rgbt bit for bit.  No float atomics: two calls give identical bits.
 * num_gaussians == 0 is TN_OK: tn_splat_bin left every tile list empty, and every pixel receives background4 (clamped to <= 1).  Refuses a null
 * pointer, a bad camera, a num_gaussians outside [0, 2^31), a negative max_intersections and a min_opacity_diff that is negative or NaN. */
TN_API int tn_splat_raster_removal_sep(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                       const float* background4, float min_opacity_diff, float* out_removal, tn_stream_t stream);

/* ---- N4 crop box: the oriented box of the eval render (SplatfactoModel.crop_box / get_outputs_for_camera, nerfstudio/models/splatfacto.py:
 * 374-376, 690-698, 904-915; OrientedBox.within, nerfstudio/data/scene_box.py:82-114).  The reference gathers the six parameter tensors
 * through a boolean index before projecting; here the test sits inside the projection kernel.  world_to_box = rows of the 3x4 matrix
 * inverse([R|T]) (the caller inverts, once, in float64, and rounds to fp32); half_extent = S / 2.  A point p is inside iff
 * |q_i| < half_extent[i] for i = 0, 1, 2 -- strict on both sides, so a point exactly on a face is outside, a non-positive extent keeps nothing,
 * and a NaN keeps nothing -- where, in fp32 with every product and sum rounded on its own (no fused multiply-add) and in this order,
 *   q_i = ((world_to_box[4i] * p.x + world_to_box[4i+1] * p.y) + world_to_box[4i+2] * p.z) + world_to_box[4i+3]. */
typedef struct TnSplatCrop {
  float world_to_box[12];
  float half_extent[3];
} TnSplatCrop;
/* the same box test on a bare point list: means [n,3] fp32 -> mask [n] uint8 (1 inside, 0 outside).  n == 0 is TN_OK; refuses a null box, null
 * pointers for n > 0 and n outside [0, 2^31). */
TN_API int tn_splat_crop_mask(const TnSplatCrop* crop, const float* means, int64_t n, uint8_t* mask, tn_stream_t stream);

/* ---- N4 pose refinement: camera-pose gradients of the training render (CameraOptimizer, nerfstudio/cameras/camera_optimizers.py:89-213, as
 * ThermalNerfactoModel uses it for both spectra, models/thermal_nerfacto.py:132-144).  A pose row p = (t, w) in R^6 -- translation, then the so(3)
 * vector -- gives A(p) = [R(w) | t] = exp_map_SO3xR3 (cameras/lie_groups.py:24-58, theta = sqrt(clamp(|w|^2, 1e-4))), applied as
 * c2w' = c2w [A(p); 0 0 0 1] (apply_to_camera, :178-186).  With F = diag(1, -1, -1) and V0 = camera->viewmat that is view' = D V0 with the rigid
 * D = F A(p)^-1 F.  The pose stays on the device: tn_splat_pose_camera writes the corrected camera into a record of
 * TN_SPLAT_POSE_CAMERA_FLOATS floats, tn_splat_project and tn_splat_project_backward read their camera from it.  Record: [0..11] view' (3x4 rows), [12..27] proj' (4x4
 * rows; row 2 is not read and is 0), [28..30] position' = c2w'[:3, 3] (the SH view directions; a value, no gradient: splatfacto.py:770),
 * [31] proj_x, [32] proj_y, the rest 0.  Everything additive: no other entry point changes.
 *
 * tn_splat_pose_camera: camera = the frame's camera as without a pose; proj_x, proj_y = entries [0][0] and [1][1] of
 * projection_matrix(0.001, 1000, fovx, fovy) (the intrinsic part of camera->projmat: proj' rows 0, 1, 3 = proj_x view'[0], proj_y view'[1],
 * view'[2]); pose_row [6] and pose_camera [TN_SPLAT_POSE_CAMERA_FLOATS] are DEVICE pointers.  One launch, nothing read back.  With a zero row every
 * number of the record equals the corresponding number of `camera` (D is exactly the identity and zero terms are skipped, not added). */
#define TN_SPLAT_POSE_CAMERA_FLOATS 40
TN_API int tn_splat_pose_camera(const TnSplatCamera* camera, float proj_x, float proj_y, const float* pose_row, float* pose_camera, tn_stream_t stream);
/* scratch of the pose backward: one partial sum of dL/d view' (12 doubles) per block of 256 Gaussians; -1 on a bad count */
TN_API int64_t tn_splat_pose_workspace_bytes(int64_t num_gaussians);

/* ---- N4 depth gradient: the training render's depth image as a differentiable output (splatfacto's training depth carries gradients,
 * nerfstudio/models/splatfacto.py:805-820).  Classic mode only.  There depth = D / A where A = accumulation > 0, with D = sum alpha_i T_i z_i on
 * the RGB chain (in separate mode too) and z_i = depths[i]; elsewhere depth is the frame's maximum of D, a value without gradient (the reference's
 * .detach().max()).  With v_depth [H,W] = dL / d depth, per pixel vD = v_depth / A (0 where A == 0): z rides the RGB chain's walk as a fifth colour
 * channel with upstream vD and no background term, and v_alpha becomes v_alpha - vD * depth.  The pair record grows by one sum, d z, reduced as the
 * others are (lane, fixed butterfly, LDS, four waves in order, one write): no float atomics, bit-reproducible.  In antialiased mode the depth is
 * blended by a chain of its own with the uncompensated opacity, whose final transmittance and last contributor the training forward does not keep:
 * tn_splat_raster_backward and tn_splat_project_backward refuse their depth groups with antialiased != 0. */

/* ---- N4 training loss: splatfacto's (1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) (nerfstudio/models/splatfacto.py:863-903), SSIM as
 * pytorch_msssim computes it: an 11-tap Gaussian window (sigma 1.5) applied separably as a VALID correlation, C1 = 0.01^2, C2 = 0.03^2 (data
 * range 1), mean over the (H-10) x (W-10) valid pixels and the channels.  L1 = mean |pred - gt| over all H W C values.  Deterministic: no
 * float atomics, the same inputs give bit-identical loss and gradient.  No host synchronisation.
 *
 * scratch of tn_image_loss: per-block partial sums and the SSIM's three per-pixel derivative maps; -1 on bad sizes (H or W < 11, channels
 * outside 1..4) */
TN_API int64_t tn_image_loss_workspace_bytes(int32_t height, int32_t width, int32_t channels);
/* pred / gt: [H,W,*] fp32 images whose pixels are pred_pixel_stride / gt_pixel_stride floats apart (rows W strides apart; channels 0..C-1 of
 * each pixel are read, so an [H,W,4] buffer serves C = 3 with stride 4).  out_loss: DEVICE [3] = weight * main loss, L1, SSIM.  out_grad:
 * [H,W,C] contiguous = d out_loss[0] / d pred (the ground truth gets none), or NULL for the loss alone.  Refused with TN_EINVAL before any
 * launch: null pointers, H or W < 11 or > 32768, channels outside 1..4, a pixel stride below the channel count, a short workspace. */
TN_API int tn_image_loss(const float* pred, int64_t pred_pixel_stride, const float* gt, int64_t gt_pixel_stride, int32_t height, int32_t width,
                         int32_t channels, float ssim_lambda, float weight, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_grad,
                         tn_stream_t stream);
/* ---- N4 thermal regularisers: ThermalNeRF's two image-space terms on the thermal render of an RGB camera -- tv_pixel_loss and
 * cross_channel_loss (nerfstudio/model_components/losses.py:602-651, used at models/thermal_nerfacto.py:346-354 on the rays with
 * is_thermal == 0) -- applied to the batch of all (H-1) x (W-1) overlapping 2 x 2 windows of one frame: stride 1, row-major, each window flattened
 * as (top-left, top-right, bottom-left, bottom-right).  With p the window of the thermal prediction and q that of the mean over the channels of
 * the RGB ground truth:
 *   tv = 0.25 * mean_w(|p0-p1| + |p0-p2| + |p1-p3| + |p2-p3|)
 *   cc = 0.25 * mean_w(|(p1-p0)-(q1-q0)| + |(p2-p0)-(q2-q0)| + |(p3-p1)-(q3-q1)| + |(p3-p2)-(q3-q2)|)
 * (the reference samples disjoint patches; stride 1 regularises every adjacent pixel pair of the frame).  One pass over the frame and a finishing
 * reduction.  Deterministic: no float atomics -- every pixel gathers its gradient from its own edges, the per-block partial sums are added in a
 * fixed order -- so the same inputs give bit-identical loss and gradient.  No host synchronisation.  A multiplier of exactly 0 skips that term's
 * arithmetic (and, for cross_mult, every read of gt_rgb): its loss is exactly 0 and it adds nothing to the gradient.
 *
 * scratch of tn_thermal_reg: the per-block partial sums; -1 on bad sizes (H or W < 2 or > 32768) */
TN_API int64_t tn_thermal_reg_workspace_bytes(int32_t height, int32_t width);
/* pred_thermal: [H,W,*] fp32 whose pixels are pred_pixel_stride floats apart (channel 0 of each pixel is read, so channel 3 of an [H,W,4] render
 * serves with stride 4); gt_rgb: [H,W,*] fp32, pixels gt_pixel_stride floats apart, channels 0..2 read; rows W strides apart in both.  out_loss:
 * DEVICE [2] = tv_mult * tv, cross_mult * cc.  out_grad: [H,W] contiguous = d (out_loss[0] + out_loss[1]) / d pred_thermal with sign(0) = 0 (the
 * ground truth gets none), or NULL for the losses alone.  Refused with TN_EINVAL before any launch: null pointers, H or W < 2 or > 32768, a pixel
 * stride below the channel count (1 for pred_thermal, 3 for gt_rgb), a short workspace. */
TN_API int tn_thermal_reg(const float* pred_thermal, int64_t pred_pixel_stride, const float* gt_rgb, int64_t gt_pixel_stride, int32_t height,
                          int32_t width, float tv_mult, float cross_mult, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_grad,
                          tn_stream_t stream);
/* ---- N4 depth losses: two geometric priors on the depth render, both only where the render is covered (accumulation > 0):
 *   depth_loss    = mean |depth - depth_image| over the pixels with accumulation > 0 and a finite, positive depth_image (a sensor depth in scene
 *                   units, nerfstudio's DepthDataset key); 0 without such a pixel, and with a null depth_image
 *   depth_tv_loss = the 2 x 2 total variation above, 0.25 * mean_w(|p0-p1| + |p0-p2| + |p1-p3| + |p2-p3|), of the depth over the stride-1 windows
 *                   whose four pixels all have accumulation > 0 (an uncovered pixel holds the frame's fill value: it would put an edge on every
 *                   silhouette); 0 without such a window
 * The two normalisations are data, so the gradient's constants exist only after the sums: a pass of partial sums and counts, a finishing reduction
 * (double, fixed order), and -- with out_grad -- a second pass in which every pixel gathers its gradient.  Deterministic: no float atomics.  No host
 * synchronisation.  A multiplier of exactly 0 skips its term: the loss is exactly 0 and adds nothing to the gradient.
 *
 * scratch of tn_depth_loss: per-block partial sums and counts, and the two gradient constants; -1 on bad sizes (H or W < 2 or > 32768) */
TN_API int64_t tn_depth_loss_workspace_bytes(int32_t height, int32_t width);
/* depth, accumulation: [H,W] fp32 contiguous; depth_image: [H,W] fp32 contiguous or NULL.  out_loss: DEVICE [2] = depth_mult * depth_loss,
 * tv_mult * depth_tv_loss.  out_grad: [H,W] contiguous = d (out_loss[0] + out_loss[1]) / d depth with sign(0) = 0 (accumulation and depth_image get
 * none), or NULL for the losses alone.  Refused with TN_EINVAL before any launch: null pointers, H or W < 2 or > 32768, a negative multiplier, a
 * short workspace. */
TN_API int tn_depth_loss(const float* depth, const float* accumulation, const float* depth_image, int32_t height, int32_t width, float depth_mult,
                         float tv_mult, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_grad, tn_stream_t stream);
/* ---- N4 per-frame colour correction: bilateral grids ("Bilateral Guided Radiance Field Processing"; gsplat's bil_grids, current splatfacto's
 * use_bilateral_grid).  grids: [F, K, L, GH, GW] fp32 contiguous, one row per frame, K = C (C + 1): for C = 3 a row-major 3 x 4 affine matrix
 * [A | b] per vertex, for C = 1 a gain and an offset.  Pixel (i, j) of an [H,W,C] image reads row `row` at
 *   x = (j + 0.5) / W,  y = (i + 0.5) / H,  g = 0.299 r + 0.587 g + 0.114 b  (C = 1: the value itself)
 * with grid coordinates (x (GW - 1), y (GH - 1), g (L - 1)), each clamped to [0, size - 1], cell = floor, the upper neighbour's index clamped to
 * size - 1 -- torch's grid_sample(mode="bilinear", padding_mode="border", align_corners=True) at 2 (x, y, g) - 1 -- the K coefficients interpolated
 * trilinearly as nested lerps a + t (b - a) (x, then y, then g; uncontracted), and out = A pixel + b.  A grid constant over a cell is reproduced
 * exactly: the identity grid returns the image's bits.  The backward gives d / d image -- A^T v plus the path through g: the coefficients' slope
 * along the third axis times L - 1 (0 where g (L - 1) is at or beyond the clamp, grid_sample's rule) times the luma weights -- and the WHOLE
 * gradient of the one grid row, every entry, exact zeros where no pixel reaches: a gather, one block per vertex, row slice and 8 levels, summed in
 * a fixed order.  Deterministic: no float atomics, the same inputs give identical bits.  No host synchronisation.
 * Sizes: C is 1 or 3; every grid side in 2..256; image sides in 1..32768; 1 <= F <= 2^20.
 *
 * scratch of tn_bilagrid_slice_backward: the row slices' partial grid gradients; -1 on sizes outside those ranges */
TN_API int64_t tn_bilagrid_workspace_bytes(int32_t channels, int32_t grid_w, int32_t grid_h, int32_t grid_l, int32_t height, int32_t width);
/* image: [H,W,*] fp32 whose pixels are pixel_stride floats apart (rows W strides apart; channels 0..C-1 of each pixel are read, so rgbt[..., :3] and
 * rgbt[..., 3:] of an [H,W,4] render are read in place).  out: [H,W,C] contiguous.  Refused with TN_EINVAL before any launch: null pointers, sizes
 * outside the ranges above, row outside 0..F-1, a pixel stride below the channel count. */
TN_API int tn_bilagrid_slice(const float* grids, int32_t num_frames, int32_t row, int32_t channels, int32_t grid_w, int32_t grid_h, int32_t grid_l,
                             const float* image, int64_t pixel_stride, int32_t height, int32_t width, float* out, tn_stream_t stream);
/* v_out: [H,W,C] contiguous, d loss / d out.  v_image: [H,W,C] contiguous.  v_grid: [K,L,GH,GW], the gradient of row `row` alone (the other rows'
 * is zero and is not written here).  Refused as above, and for a short workspace. */
TN_API int tn_bilagrid_slice_backward(const float* grids, int32_t num_frames, int32_t row, int32_t channels, int32_t grid_w, int32_t grid_h,
                                      int32_t grid_l, const float* image, int64_t pixel_stride, int32_t height, int32_t width, const float* v_out,
                                      void* workspace, int64_t workspace_bytes, float* v_image, float* v_grid, tn_stream_t stream);
/* The grids' total variation, gsplat's total_variation_loss: for each of the three grid axes the sum of squared first differences along it divided
 * by the number of entries of ONE frame's difference tensor (K L GH (GW - 1) for x), the three terms added and divided by F.
 * scratch of tn_bilagrid_tv: one partial sum per block; -1 on bad sizes (sides as above, 1..64 coefficients, at most 2^34 entries in all) */
TN_API int64_t tn_bilagrid_tv_workspace_bytes(int32_t num_frames, int32_t coefficients, int32_t grid_w, int32_t grid_h, int32_t grid_l);
/* out: DEVICE [1] = mult * tv.  out_grad: [F,K,L,GH,GW] = d out / d grids, written in the same call, or NULL for the value alone.  Every entry gathers
 * its six neighbours; partial sums are added in a fixed order (double).  Constant grids give exactly 0. */
TN_API int tn_bilagrid_tv(const float* grids, int32_t num_frames, int32_t coefficients, int32_t grid_w, int32_t grid_h, int32_t grid_l, float mult,
                          void* workspace, int64_t workspace_bytes, float* out, float* out_grad, tn_stream_t stream);
/* ---- N4 resolution schedule: bilinear resize of one image, what splatfacto's _downscale_if_required does with
 * torchvision.transforms.functional.resize(antialias=None) (nerfstudio/models/splatfacto.py:648-657), i.e. torch.nn.functional.interpolate(
 * mode="bilinear", align_corners=False, antialias=False).  Per axis: scale = (float)in / out, source coordinate scale * (dst + 0.5) - 0.5 clamped
 * below at 0, taps i0 = floor(src) and i1 = min(i0 + 1, in - 1), weight of i1 = src - i0; interpolation along x, then along y, all in fp32.  Shrinking
 * and enlarging follow the same formula.  Deterministic; no workspace, no host synchronisation.
 *
 * in: [in_height, in_width, *] of in_dtype whose pixels are in_pixel_stride ELEMENTS apart (rows in_width strides apart; channels 0..C-1 of each
 * pixel are read).  A TN_IMAGE_U8 value v enters as (float)v / 255.0f, so the result has the bits of resizing the pre-divided fp32 image.
 * out: [out_height, out_width, C] fp32, contiguous.  Refused with TN_EINVAL before any launch: null pointers, an unknown in_dtype, channels
 * outside 1..4, a pixel stride below the channel count, a side below 1 or above 32768. */
#define TN_IMAGE_F32 0
#define TN_IMAGE_U8 1
TN_API int tn_image_resize(const void* in, int32_t in_dtype, int64_t in_pixel_stride, int32_t in_height, int32_t in_width, int32_t channels,
                           float* out, int32_t out_height, int32_t out_width, tn_stream_t stream);
/* ---- N4 undistortion: one distorted training frame resampled into the pinhole frame the rasteriser renders, what the reference's
 * FullImageDatamanager does once per frame with OpenCV (data/datamanagers/full_images_datamanager.py:351-386).  The distortion model is tn_raygen's
 * (k = k1 k2 k3 k4 p1 p2, the dataparser's order): with r = x^2 + y^2, d = 1 + r (k1 + r (k2 + r (k3 + r k4))),
 * x_d = d x + 2 p1 x y + p2 (r + 2 x^2), y_d = d y + 2 p2 x y + p1 (r + 2 y^2); pixel (u, v) has its centre at (u + 0.5, v + 0.5), as in tn_raygen
 * and the splat rasteriser.  Output pixel (u, v): x = (u + 0.5 - new_cx) / new_fx, y = (v + 0.5 - new_cy) / new_fy, the polynomial above (closed
 * form, no iteration), source position s = (fx x_d + cx - 0.5, fy y_d + cy - 0.5) clamped to [-1, width] x [-1, height], taps floor(s) and
 * floor(s) + 1 with their indices clamped to the frame, weight of the second s - floor(s); interpolation along x, then along y, all in fp32.
 * Deterministic; no workspace, no host synchronisation.  The caller chooses the new intrinsics (splat.undistorted_camera: the largest pinhole frame
 * of the same size that reads only inside the source). */
typedef struct TnUndistort {
  float fx, fy, cx, cy;                 /* the source frame's (distorted) camera */
  float new_fx, new_fy, new_cx, new_cy; /* the output frame's pinhole camera */
  float k[6];                           /* k1 k2 k3 k4 p1 p2 */
} TnUndistort;
/* in: [height, width, *] of in_dtype whose pixels are in_pixel_stride ELEMENTS apart (rows width strides apart; channels 0..C-1 of each pixel are
 * read).  A TN_IMAGE_U8 value v enters as (float)v / 255.0f.  out: [height, width, C] of out_dtype, contiguous; a TN_IMAGE_U8 output is
 * rintf(255 * clamp(value, 0, 1)).  in and out must not overlap.  Refused with TN_EINVAL before any launch: null pointers, an unknown in_dtype or
 * out_dtype, channels outside 1..4, a pixel stride below the channel count, a side below 1 or above 32768, a focal length that is not finite and
 * positive, a non-finite principal point or coefficient. */
TN_API int tn_image_undistort(const void* in, int32_t in_dtype, int64_t in_pixel_stride, int32_t height, int32_t width, int32_t channels, void* out,
                              int32_t out_dtype, const TnUndistort* params, tn_stream_t stream);
/* ---- N4 seeding: exact k-nearest-neighbour distances over a point cloud (splatfacto's k_nearest_sklearn, nerfstudio/models/splatfacto.py:272-290,
 * which seeds each Gaussian's log-scale from the mean distance to its 3 nearest neighbours).  Row i of out_dist holds the k smallest distances
 * from point i to the points j != i, ascending; a duplicate of point i is a neighbour at distance 0.  d2 = (dx*dx + dy*dy) + dz*dz with
 * dx = xi - xj (and dy, dz) in fp32, each operation rounded, distance = sqrtf(d2) correctly rounded; ties on d2 go to the smaller index.  The
 * result is exact -- bit-identical to a brute force with that formula -- and deterministic (no float atomics).  No host synchronisation.
 *
 * scratch of tn_knn; -1 on bad sizes (n outside 0..INT32_MAX, k outside 1..8) or when the sort's scratch cannot be sized (no device) */
TN_API int64_t tn_knn_workspace_bytes(int64_t n, int32_t k);
/* points [n,3] fp32 -> out_dist [n,k] and, unless NULL, out_index [n,k] int32 (the neighbours' row numbers).  n == 0 does nothing.  Refused with
 * TN_EINVAL before any launch: k outside 1..8, n < 0 or n > INT32_MAX, null pointers, n < k + 1, a short workspace. */
TN_API int tn_knn(const float* points, int64_t n, int32_t k, float* out_dist, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                  tn_stream_t stream);

/* ---- N4 training, MCMC strategy (ThermalSplatfactoModelConfig.strategy = "mcmc": "3D Gaussian Splatting as Markov Chain Monte Carlo", gsplat's
 * MCMCStrategy): a fixed budget of Gaussians; dead ones are moved onto live ones, the population grows to its cap, and position noise keeps the
 * faint ones exploring.  tests/splat_mcmc_functional.py restates both operations in float64.
 *
 * tn_splat_mcmc_relocate: num_draws draws (src_idx[j] -> dst_idx[j]; both DEVICE int64 [num_draws]) on tensors of num_rows rows, in place.
 * params / exp_avg / exp_avg_sq: HOST arrays of num_tensors device pointers (8 or 9; anything else is refused) in tn_splat_refine_apply's order
 * (K = num_rest_coeffs; the two rest entries are ignored when K = 0; ninth, opacities_thermal [N,1]: the thermal opacity takes its own o_th' by the
 * rule below, and the scale follows the larger of the two opacities, a tie going to o); a parameter's two moment pointers are both null (no Adam
 * state) or both set.  With ratio r = min(1 + the number of times a
 * source row was drawn, 51), o = sigmoid(opacity) and s = exp(log-scale) of the source BEFORE the call:
 *   o' = clamp(1 - (1 - o)^(1/r), min_opacity, 1 - FLT_EPSILON), stored as log(o' / (1 - o'));
 *   p' = 1 - (1 - o)^(1/r) unclamped, denom = sum_{i=1..r} sum_{k=0..i-1} binom(i-1, k) (-1)^k p'^(k+1) / sqrt(k+1), s' = (o / denom) s, stored as
 *   log s', on all three axes -- evaluated in double from the fp32 inputs and rounded once (r = 1: the identity up to the clamp).
 * Every drawn source row takes (o', s') once, however often it was drawn, and both Adam moments of that row become zero in every tensor.  Every
 * destination row becomes a copy of its source's row in every tensor, with (o', s'); its moments stay what they were.  Rows not named are
 * untouched.  The caller's rule: no destination is also a source, no destination repeats (relocation: the dead rows; growth: rows appended with
 * zero moments before the call).  A draw with an index outside [0, num_rows) is skipped.  The draw counts use integer atomics on the zeroed
 * workspace, so the result is bit-reproducible.  No host synchronisation.  num_draws == 0 launches nothing.  Refused with TN_EINVAL before any
 * launch: num_rows or num_draws negative or above INT32_MAX, draws on no rows, K outside 0..15, min_opacity outside (0, 1), null pointers, partly
 * null moments, a short workspace.
 *
 * scratch of tn_splat_mcmc_relocate (a counter and five values per row, a flag per draw); -1 on bad sizes */
TN_API int64_t tn_splat_mcmc_workspace_bytes(int64_t num_rows, int64_t num_draws);
TN_API int tn_splat_mcmc_relocate(int64_t num_rows, int32_t num_rest_coeffs, const int64_t* src_idx, const int64_t* dst_idx, int64_t num_draws,
                                  float min_opacity, int32_t num_tensors, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                  void* workspace, int64_t workspace_bytes, tn_stream_t stream);
/* The position noise of one training step, in place: means [N,3] += Sigma (randn * g * scaler) with Sigma = R diag(exp(log_scales)^2) R^T,
 * R the rotation of quats / |quats| (w x y z, the projection's convention), g = 1 / (1 + exp(-100 ((1 - o) - 0.995))), o = sigmoid(opacities) -- or, with
 * opacities_thermal (optional), the larger of the two sigmoids: a Gaussian visible in either spectrum is left in place --,
 * randn [N,3] standard normal draws, scaler = noise_lr times the means' learning rate.  One launch, one thread per Gaussian, fp32, no [N,3,3]
 * temporary; memory-bound at 68 bytes per Gaussian.  quats must be 16-byte aligned.  num_gaussians == 0 launches nothing.  Refused with TN_EINVAL
 * before any launch: a count that is negative or above INT32_MAX, null pointers, a scaler that is negative or not finite. */
TN_API int tn_splat_mcmc_noise(float* means, const float* log_scales, const float* quats, const float* opacities, const float* opacities_thermal,
                               const float* randn, int64_t num_gaussians, float scaler, tn_stream_t stream);

/* ---- Gaussian-splat PLY export (ns-export gaussian-splat: nerfstudio/scripts/exporter.py:480-546, ExportGaussianSplat): the model's parameter
 * tensors become the rows of an Inria-layout splat file on the device, filtered and compacted in their original order.  Runs on the caller's
 * stream without a host synchronisation and without atomics: the same inputs give the same bytes.  tests/splat_export_functional.py restates it.
 *
 * tn_export_splat_pack: the parameters as tn_splat_project takes them -- means, log_scales [N,3], quats [N,4] (written as stored, not
 * normalised), opacities [N] (logits), features_dc [N,3], features_rest [N,R,3], thermal_dc [N], thermal_rest [N,R] with R = num_rest_coeffs (the
 * two rest tensors may be null when R is 0), opacities_thermal [N] or null (shared opacity).  spectrum: 0 rgb, 1 thermal, 2 both.  The row of W
 * floats, with o = 9 + 3 R:
 *   0..2 x y z | 3..5 nx ny nz = 0 | 6..8 f_dc_0..2 | 9..o-1 f_rest_{c R + k} = features_rest[g,k,c] (channel-major) | o opacity |
 *   o+1..o+3 scale_0..2 | o+4..o+7 rot_0..3                                                             W = 17 + 3 R for rgb and thermal
 *   thermal: the same columns with f_dc_c = thermal_dc[g], f_rest_{c R + k} = thermal_rest[g,k], opacity = opacities_thermal[g] where given, else
 *   opacities[g] -- a grey scene under the Inria property names;
 *   both: the rgb row, then o+8 f_dc_thermal | o+9..o+8+R f_rest_thermal_0..R-1 | with opacities_thermal, o+9+R opacity_thermal.
 * colour_mode 0 writes the SH coefficients as stored; colour_mode 1 (the model's sh_degree == 0 convention, colour = sigmoid(dc); R must be 0)
 * writes f_dc = (sigmoid(dc) - 0.5) / 0.28209479177387814 in double, rounded once, also for f_dc_thermal.
 * Gaussian g is kept iff
 *   every parameter its row is made of is finite (a thermal-only parameter does not matter to an rgb row, nor an RGB-only one to a thermal row), and
 *   the opacity logit of the row >= min_opacity_logit (a float compare; -inf switches it off; with two logits in the row, the larger of them), and
 *   crop is null, or the mean is inside the box exactly as tn_splat_crop_mask tests it.  crop is a HOST pointer, read before the launch.
 * The kept rows go to out_rows [N, W] in the Gaussians' order, count (DEVICE int64[1]) is SET to their number, rows at and beyond it are not
 * written.  num_gaussians == 0 is TN_OK and sets count to 0.  Refused with TN_EINVAL before any launch: num_gaussians outside [0, 2^31),
 * num_rest_coeffs negative or above 1024, an unknown spectrum or colour_mode, colour_mode 1 with num_rest_coeffs > 0, a NaN threshold, null
 * pointers, a workspace that is short or not 8-byte aligned.
 *
 * scratch of tn_export_splat_pack (a keep flag per Gaussian, a count and an offset per block of 256); -1 for num_gaussians outside [0, 2^31) */
TN_API int64_t tn_export_splat_workspace_bytes(int64_t num_gaussians);
TN_API int tn_export_splat_pack(const float* means, const float* log_scales, const float* quats, const float* opacities, const float* features_dc,
                                const float* features_rest, const float* thermal_dc, const float* thermal_rest, const float* opacities_thermal,
                                int64_t num_gaussians, int32_t num_rest_coeffs, int32_t spectrum, int32_t colour_mode, float min_opacity_logit,
                                const TnSplatCrop* crop, float* out_rows, int64_t* count, void* workspace, int64_t workspace_bytes,
                                tn_stream_t stream);

/* ---- a rigid move of the Gaussians: the similarity x' = s R x + t (s > 0, R a proper rotation) applied to every Gaussian, so that the moved
 * model seen from the moved camera renders the same frame -- what an export to, or an import from, the dataset's frame needs.  One launch on the
 * caller's stream, no atomics, no workspace, no host synchronisation; the same inputs give the same bytes.  tests/splat_transform_functional.py
 * restates it.
 *
 * TnSplatTransform is filled on the host in double (nerfstudio_thermal_amd.splat_transform.transform_struct): A = s R row-major, t, log_scale =
 * log s, q = the quaternion (w, x, y, z) of R, and sh1 [3,3], sh2 [5,5], sh3 [7,7] row-major, the rotation matrices of the real SH bands 1 to 3 in
 * tn_splat_project's basis (gsplat's constants, order and signs): Y_l(R d) = sh_l Y_l(d).
 *
 * tn_transform_splat: means, log_scales [N,3], quats [N,4] as stored, features_rest [N,R,3], thermal_rest [N,R] with R = num_rest_coeffs in
 * {0, 3, 8, 15} (degrees 0 to 3; with R = 0 only the geometry moves and the four rest pointers may be null).  Every output value is evaluated in
 * double from the float inputs widened, in this order, and rounded once to float:
 *   means'[i]  = ((A[i][0] x + A[i][1] y) + A[i][2] z) + t[i]
 *   scales'[i] = scales[i] + log_scale
 *   quats'     = q (x) quat, the Hamilton product, each component the left-to-right sum of its four products:
 *                w' = ((w1 w2 - x1 x2) - y1 y2) - z1 z2      x' = ((w1 x2 + x1 w2) + y1 z2) - z1 y2
 *                y' = ((w1 y2 - x1 z2) + y1 w2) + z1 x2      z' = ((w1 z2 + x1 y2) - y1 x2) + z1 w2      (1: q, 2: the Gaussian's; its norm is kept)
 *   rest'[k]   = ((M[k][0] rest[0] + M[k][1] rest[1]) + ...), j ascending, within each band present (k = 0..2 with sh1, 3..7 with sh2, 8..14 with
 *                sh3), per channel, for features_rest and thermal_rest alike
 * A parameter that is not finite leaves its group (means, scales, quats, a band of a channel) of its Gaussian not finite.
 * Each *_out may be its own input (in place): a block reads all of its Gaussians before it stores any.  Otherwise an output must not overlap any
 * other buffer of the call: pointers are equal or disjoint.
 * num_gaussians == 0 is TN_OK without a launch.  Refused with TN_EINVAL before any launch: a null transform, num_gaussians outside [0, 2^31),
 * num_rest_coeffs not one of 0, 3, 8, 15, null pointers the call needs. */
typedef struct TnSplatTransform {
  double A[9];
  double t[3];
  double log_scale;
  double q[4];
  double sh1[9], sh2[25], sh3[49];
} TnSplatTransform;
TN_API int tn_transform_splat(const TnSplatTransform* transform, const float* means, const float* log_scales, const float* quats,
                              const float* features_rest, const float* thermal_rest, int64_t num_gaussians, int32_t num_rest_coeffs,
                              float* means_out, float* log_scales_out, float* quats_out, float* features_rest_out, float* thermal_rest_out,
                              tn_stream_t stream);

/* ---- Mip-Splatting's 3D smoothing filter (ThermalSplatfactoModelConfig.use_3d_filter; "Mip-Splatting: Alias-free 3D Gaussian Splatting", eq. 6-7
 * and 9): every Gaussian is band-limited to the highest frequency any training camera could have sampled, as a per-Gaussian pre-transform of the
 * log-scales and opacity logits the rasteriser reads.  Everything runs on the caller's stream without atomics, host synchronisation or read-back;
 * every value is evaluated in double from the float inputs widened and rounded once; the same inputs give the same bits.
 * tests/splat_filter3d_functional.py restates all three.
 *
 * tn_filter3d_splat_compute: means [N,3], cameras [num_cameras,18] fp32 -- per row the 12 entries of the world -> camera matrix in
 * TnSplatCamera.viewmat's convention, then fx, fy, cx, cy, width, height -> filter_3d [N].  With (x, y, z) = viewmat [p; 1], each coordinate
 * ((m0 px + m1 py) + m2 pz) + m3, u = fx x / z + cx and v = fy y / z + cy, camera n sees Gaussian k iff z > near_plane and
 * -0.15 width <= u <= 1.15 width and -0.15 height <= v <= 1.15 height.  nu_k = the maximum of max(fx, fy) / z over the cameras that see k, and
 * filter_3d[k] = sqrt(variance) / nu_k.  A Gaussian no camera sees takes the smallest nu of the seen ones (the largest filter); when no Gaussian is
 * seen (or num_cameras == 0) every row is 0: the filter is off.  The maximum is taken per camera as the paper states it, NOT by the official code's
 * shortcut of one global focal length over each Gaussian's smallest depth, which is wrong by the ratio of the focal lengths on a rig whose
 * cameras differ (a thermal camera at a quarter of the RGB resolution).  Two launches: per-block minima of nu go to the workspace, the second
 * launch folds them and writes the unseen rows.  num_gaussians == 0 is TN_OK without a launch.  Refused with TN_EINVAL before any launch:
 * num_gaussians outside [0, 2^31), num_cameras < 0, near_plane or variance negative or not finite, null pointers, a workspace that is short or not
 * 8-byte aligned.
 *
 * scratch of tn_filter3d_splat_compute (a double per block of 256 Gaussians); -1 on bad sizes */
TN_API int64_t tn_filter3d_splat_workspace_bytes(int64_t num_gaussians);
TN_API int tn_filter3d_splat_compute(const float* means, int64_t num_gaussians, const float* cameras, int32_t num_cameras, double near_plane,
                                     double variance, float* filter_3d, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
/* log_scales [N,3], opacities [N] (logits), opacities_thermal [N] or NULL, filter_3d [N] -> the scales and opacities the rasteriser is to read.
 * With f = filter_3d[k], s_i = exp(log_scales[k][i]), r_i = s_i^2 / (s_i^2 + f^2), c = sqrt(r_0 r_1 r_2) -- evaluated as log c = -1/2 ((log1p(t_0) +
 * log1p(t_1)) + log1p(t_2)), t_i = f^2 / s_i^2, and 1 - c = -expm1(log c), so that 1 - c does not cancel where f is far below the scales:
 *   log_scales_out[k][i] = 1/2 log(s_i^2 + f^2)          opacities_out[k] = (o + log c) - log1p(e^o (1 - c))   (the logit of sigmoid(o) c)
 * and opacities_thermal_out likewise from opacities_thermal.  A row with f == 0 is copied bit for bit.  One launch, a thread per Gaussian.  The two
 * thermal pointers are both NULL (shared mode) or both set.  An output may be its own input.  Refused with TN_EINVAL before any launch:
 * num_gaussians outside [0, 2^31), null pointers, a thermal pointer pair that is half set. */
TN_API int tn_filter3d_splat_apply(const float* log_scales, const float* opacities, const float* opacities_thermal, const float* filter_3d,
                                   int64_t num_gaussians, float* log_scales_out, float* opacities_out, float* opacities_thermal_out,
                                   tn_stream_t stream);
/* The exact derivative of tn_filter3d_splat_apply in the raw log-scales and logits (filter_3d takes none), closed form, one launch.  With
 * 1 - p = 1 / (1 + e^o), p = 1 / (1 + e^-o), 1 - p' = (1 - p) + p (1 - c), 1 - r_i = f^2 / (s_i^2 + f^2), per chain:
 *   v_log_scales[k][i] = v_log_scales_out[k][i] r_i + (v_opacities_out[k] / (1 - p') + v_opacities_thermal_out[k] / (1 - p'_th)) (1 - r_i)
 *   v_opacities[k]     = v_opacities_out[k] (1 - p) / (1 - p')                              (and the thermal chain's likewise)
 * A row with f == 0 copies its upstream gradients bit for bit.  The three thermal pointers are all NULL or all set. */
TN_API int tn_filter3d_splat_apply_backward(const float* log_scales, const float* opacities, const float* opacities_thermal, const float* filter_3d,
                                            const float* v_log_scales_out, const float* v_opacities_out, const float* v_opacities_thermal_out,
                                            int64_t num_gaussians, float* v_log_scales, float* v_opacities, float* v_opacities_thermal,
                                            tn_stream_t stream);

/* ---- ray contribution of every Gaussian (splat_prune.py: RadSplat's max over rays of alpha T, LightGaussian's hit-weighted sum), the score trained
 * splats are pruned by.  tn_splat_raster_contrib runs on the frame workspace tn_splat_project and tn_splat_bin left, exactly as tn_splat_raster
 * does, and walks ONE transmittance chain of the frame's tile lists: chain 0 is the chain RGB, accumulation and depth are blended with, chain 1
 * the thermal chain of a frame projected with opacities_thermal (only such a frame has one: the workspace does not say how it was projected,
 * the caller must).  In antialiased mode the alpha is the one the chain's colour is blended with, the compensated one; the workspace's records hold it already,
 * so `antialiased` (0 or 1, the frame's flag) is validated and selects nothing.  For every pixel p and every list entry g the forward would blend on
 * that chain -- the same power >= 0 test, 1/255 gate, 0.999 clamp and nT <= 1e-4 stop, from the rasteriser's own helpers --
 *   w = pixel_weight[p] * alpha * T          pixel_weight: [H,W] fp32, non-negative; NULL means 1
 * and a Gaussian at which a pixel stops is not blended there and scores nothing there.  Four accumulators [num_gaussians] are updated IN PLACE, so
 * a loop over cameras needs no temporaries and no read-back (the caller zeroes them before the first frame):
 *   max_acc   fp32   max(old, max over p of w)
 *   sum_acc   fp64   old + sum over p of w    (the frame's sum is formed in fp32 in a fixed order and added to the double once)
 *   hits_acc  int64  old + the number of pixels with w > 0
 *   views_acc int32  old + 1 if the frame's max is > 0
 * Three launches, no atomics, no host synchronisation: the same inputs give the same bits.  The raster writes one (sum, max, count) record per
 * (Gaussian, tile) pair into `scratch` -- every pair of every tile, zeros where nothing is blended -- and a fold per Gaussian walks its run.
 * num_gaussians == 0 is TN_OK without a launch.  Refused with TN_EINVAL before any launch: a bad camera, sizes outside [0, 2^31), antialiased or
 * chain other than 0 or 1, null pointers, a scratch shorter than tn_splat_contrib_workspace_bytes(num_gaussians, max_intersections) (-1 on bad
 * sizes).  max_intersections is the capacity the frame workspace was laid out with. */
TN_API int64_t tn_splat_contrib_workspace_bytes(int64_t num_gaussians, int64_t max_intersections);
TN_API int tn_splat_raster_contrib(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                   int32_t antialiased, int32_t chain, const float* pixel_weight, void* scratch, int64_t scratch_bytes,
                                   float* max_acc, double* sum_acc, int64_t* hits_acc, int32_t* views_acc, tn_stream_t stream);

/* ---- point-cloud export of the NeRF (ns-export pointcloud: nerfstudio/scripts/exporter.py:90-186, nerfstudio/exporter/exporter_utils.py:83-260,
 * generate_point_cloud): rendered rays are back-projected by their depth, the opaque ones inside a box are kept, statistical outliers are
 * removed.  Every point carries the rendered colour and the rendered thermal value.  Both entry points run on the caller's stream without a host
 * synchronisation and use no float atomics: the same inputs give the same bytes.  tests/cloud_functional.py restates both.
 *
 * tn_cloud_append: one batch of num_rays rendered rays.  origins, directions [num_rays,3], depth, accumulation [num_rays] fp32, contiguous;
 * rgb: channels 0..2 of ray r at rgb[r * rgb_stride], thermal: the value of ray r at thermal[r * thermal_stride] (strides in ELEMENTS, so both can
 * be read in place from one [num_rays,4] rgbt buffer: rgb = buffer, thermal = buffer + 3, both strides 4).  Ray r is kept iff
 *   accumulation[r] > alpha_thresh (strict), and
 *   p = o + d * depth[r] is finite in all three coordinates (fp32, the product and the sum each rounded on its own), and
 *   box is null, or p is inside it exactly as tn_splat_crop_mask tests it (strict on both sides; a NaN keeps nothing).
 * count: DEVICE int64[1], the rows the output holds already (read as clamped to 0..cap).  The kept rays' p, rgb and thermal are written in ray
 * order to rows count, count + 1, ... of out_xyz [cap,3], out_rgb [cap,3], out_thermal [cap]; rows at or beyond cap are dropped, nothing is
 * written there; afterwards count = min(cap, count + kept).  box is a HOST pointer, read before the launch.  The outputs must not overlap the
 * inputs.  num_rays == 0 is TN_OK and touches nothing.  Refused with TN_EINVAL before any launch: num_rays negative or at or above 2^31, a negative cap,
 * null pointers (box may be null, and so may the three outputs when cap is 0), an rgb stride below 3 or a thermal stride below 1, a short workspace.
 *
 * scratch of tn_cloud_append (a count and an offset per block of 256 rays); -1 for num_rays outside [0, 2^31) */
TN_API int64_t tn_cloud_append_workspace_bytes(int64_t num_rays);
TN_API int tn_cloud_append(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* rgb,
                           int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t num_rays, float alpha_thresh,
                           const TnSplatCrop* box, float* out_xyz, float* out_rgb, float* out_thermal, int64_t cap, int64_t* count, void* workspace,
                           int64_t workspace_bytes, tn_stream_t stream);
/* tn_cloud_remove_outliers: Open3D's remove_statistical_outlier(nb_neighbors, std_ratio) (the reference calls it with nb_neighbors = 20) over
 * xyz [n,3], rgb [n,3], thermal [n] fp32.  The rule:
 *   mean_i = (the sum of the distances from point i to its nb_neighbors - 1 nearest OTHER points, ascending, accumulated in double) / nb_neighbors
 *            -- Open3D's search returns the query itself at distance 0 as the first of the nb_neighbors; the distances are tn_knn's:
 *            d2 = (dx*dx + dy*dy) + dz*dz in fp32, sqrtf(d2), ties to the smaller index, exact;
 *   over the V points with mean_i > 0, in double: m = their mean, s = sqrt(sum (mean_i - m)^2 / (V - 1)), thr = m + std_ratio * s
 *            (V == 0 makes m, and V == 1 makes s, 0 / 0: the NaN keeps nothing);
 *   point i is kept iff mean_i > 0 && mean_i < thr.
 * The kept points' rows go to out_xyz / out_rgb / out_thermal (room for n rows each; they must not overlap the inputs) compacted in their original
 * order, their number to out_count (DEVICE int64[1]), stats = [m, s, thr] (DEVICE double[3]); unless null, mean [n] double receives every mean_i
 * and keep [n] uint8 the mask.  The sums are folded in a fixed order.  The neighbour search is the wide form of tn_knn's query on the same tree
 * (lists of 7, 15, 19 or 31 in registers); it writes mean_i only, no [n,k] table.  Refused with TN_EINVAL before any launch: nb_neighbors outside
 * 2..32, n < nb_neighbors, n at or above 2^31, null pointers (mean and keep may be null), a short workspace.
 *
 * scratch of tn_cloud_remove_outliers (tn_knn's tree, the means, the partial sums, a count and an offset per block); -1 on sizes the call refuses or
 * when the sort's scratch cannot be sized (no device) */
TN_API int64_t tn_cloud_remove_outliers_workspace_bytes(int64_t n, int32_t nb_neighbors);
TN_API int tn_cloud_remove_outliers(const float* xyz, const float* rgb, const float* thermal, int64_t n, int32_t nb_neighbors, double std_ratio,
                                    float* out_xyz, float* out_rgb, float* out_thermal, int64_t* out_count, double* stats, double* mean, uint8_t* keep,
                                    void* workspace, int64_t workspace_bytes, tn_stream_t stream);
/* The view directions beside the points, for the normals below.  tn_cloud_append_view is tn_cloud_append plus out_view [cap,3] (after out_thermal):
 * the direction of every kept ray, as given and not renormalised, goes to the row its point goes to.  tn_cloud_remove_outliers_view is
 * tn_cloud_remove_outliers plus view [n,3] (after thermal) and out_view [n,3] (after out_thermal), compacted with the points.  Both run the plain
 * entry points' launches with one more pointer pair in the write kernel, so every other output is what the plain call writes, bit for bit, and
 * everything the plain calls refuse is refused; the new pointers must not be null (out_view may be when cap is 0). */
TN_API int tn_cloud_append_view(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* rgb,
                                int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t num_rays, float alpha_thresh,
                                const TnSplatCrop* box, float* out_xyz, float* out_rgb, float* out_thermal, float* out_view, int64_t cap, int64_t* count,
                                void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_cloud_remove_outliers_view(const float* xyz, const float* rgb, const float* thermal, const float* view, int64_t n, int32_t nb_neighbors,
                                         double std_ratio, float* out_xyz, float* out_rgb, float* out_thermal, float* out_view, int64_t* out_count,
                                         double* stats, double* mean, uint8_t* keep, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
/* tn_cloud_estimate_normals: an oriented unit normal per point of xyz [n,3] (finite fp32), the rule of Open3D's estimate_normals with
 * KDTreeSearchParamKNN(knn) followed by the reference's reorient_normals (exporter_utils.py:215-237).  knn in 3..32 counts the point itself.
 *   Neighbourhood  N_i = point i, then its knn - 1 nearest OTHER points in tn_knn's order: d2 = (dx*dx + dy*dy) + dz*dz in fp32, ties to the smaller
 *                  index, exact.  A duplicate of i is a neighbour at distance 0.
 *   Covariance     in double: c_j = p_j - p_i (exact), S1 = sum c_j and S2 = sum c_j c_j^T over N_i in that order,
 *                  C = S2 / knn - (S1 / knn)(S1 / knn)^T.
 *   Normal         the unit eigenvector of C's smallest eigenvalue, rounded once to fp32.  C is scaled by its trace and diagonalised by cyclic
 *                  Jacobi rotations in double until its off-diagonal sum is at most 2^-100 (12 sweeps at the most), so the vector's error is of
 *                  the order of 2^-52 lambda_max / (lambda_1 - lambda_0).
 *   Zero C         C exactly zero (all knn points coincide): the normal is (0, 0, 1), Open3D's fallback.
 *   Sign, view     with view [n,3] (the direction of the ray that produced the point): the normal is negated when v_i . n > 0, the dot product
 *                  ((vx nx + vy ny) + vz nz) in double on the unrounded normal.
 *   Sign, no view  view null: the first non-zero of (n_z, n_y, n_x) is positive.
 * Every output is finite and of unit length, degenerate neighbourhoods included (a collinear run gives some unit vector normal to the line).
 * Nothing but out_normals[i] is written; no atomics, no host synchronisation, the same inputs give the same bits.  The search is the wide form of
 * tn_knn's query (lists of 7, 15, 19 or 31 in registers, chosen by knn - 1), the neighbours are gathered by their original indices; no [n,k] table.
 * n == 0 is TN_OK and touches nothing.  Refused with TN_EINVAL before any launch: knn outside 3..32, n < knn, n at or above 2^31, null pointers
 * (view may be null), a short workspace.  tests/cloud_normals_functional.py restates the rule.
 *
 * scratch of tn_cloud_estimate_normals (tn_knn's tree); 0 for n == 0, -1 on sizes the call refuses or when the sort's scratch cannot be sized */
TN_API int64_t tn_cloud_normals_workspace_bytes(int64_t n, int32_t knn);
TN_API int tn_cloud_estimate_normals(const float* xyz, int64_t n, int32_t knn, const float* view, float* out_normals, void* workspace,
                                     int64_t workspace_bytes, tn_stream_t stream);

/* ---- TSDF mesh export (ns-export tsdf: nerfstudio/exporter/tsdf_utils.py, TSDF.integrate_tsdf and get_mesh): rendered depth frames are fused into
 * a truncated signed distance volume with an RGB+thermal value per voxel, and the zero level of the volume is extracted as an indexed triangle mesh.
 * All three entry points run on the caller's stream without a host synchronisation and without atomics: the same inputs give the same bytes.
 * tests/tsdf_functional.py restates them.
 *
 * The volume: values [X,Y,Z] (the reference starts it at -1), weights [X,Y,Z] (at 0) and rgbt [X,Y,Z,4] (16-byte aligned), fp32, z fastest.  Voxel
 * (i, j, k) sits at origin + (i, j, k) * voxel (the product and the sum each rounded on its own).  X * Y * Z is below 2^31.
 *
 * tn_tsdf_integrate: num_frames frames in ONE launch, a thread per voxel, the frames in the order given.  depth [B,H,W], frame_rgbt [B,H,W,4]
 * (channel-last, 16-byte aligned), accumulation [B,H,W] or null, cameras [B,16] on the DEVICE: the rows of the 3x4 world -> camera matrix
 * (nerfstudio's camera: x right, y up, z back), then fx fy cx cy.  Per frame, in fp32 with every operation rounded on its own:
 *   (x, y, z) = M [p, 1] with y and z negated; a voxel with z <= 0 is skipped (the reference divides by that z and mirrors the voxel into the image);
 *   voxel depth vd = sqrt((x x + y y) + z z) with ray_depth 1 (the reference's rule, the depth of a NeRF), z with ray_depth 0 (a rasteriser's depth);
 *   pixel column = rint(fx (x / z) + cx - 0.5), row = rint(fy (y / z) + cy - 0.5), half to even: the nearest-pixel sample of
 *   grid_sample(mode="nearest", align_corners=False, padding_mode="zeros"); outside the image the sample is 0;
 *   with accumulation, a pixel whose accumulation < min_accumulation counts as depth 0;
 *   dist = depth - vd; the sample is valid iff vd > 0, depth > 0 and dist > -truncation; tsdf = clamp(dist / truncation, -1, 1);
 *   where valid: value = (value w + tsdf) / (w + 1), the same for the four rgbt channels, then w = min(w + 1, max_weight).
 * max_weight 1 is the reference (a running half-and-half average that depends on the frame order), a large one the running mean.  A voxel no frame
 * of the call observes is neither read nor written, so splitting the frames over several calls gives the same bits.  num_frames == 0 is TN_OK and
 * touches nothing.  Refused with TN_EINVAL before any launch: sizes outside the above (H, W in 1..32768), an origin that is not finite, a voxel size
 * or truncation that is not positive and finite, max_weight <= 0, ray_depth other than 0 or 1, null pointers (accumulation may be null), misaligned
 * rgbt arrays. */
TN_API int tn_tsdf_integrate(float* values, float* weights, float* rgbt, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y,
                             float origin_z, float voxel_x, float voxel_y, float voxel_z, float truncation, float max_weight, const float* depth,
                             const float* frame_rgbt, const float* accumulation, float min_accumulation, const float* cameras, int32_t num_frames,
                             int32_t height, int32_t width, int32_t ray_depth, tn_stream_t stream);
/* Surface extraction at level 0 of v = clamp(values, -1, 1) by marching tetrahedra on the Freudenthal split of each cell: with the corners of a cell
 * numbered dx + 2 dy + 4 dz, the tetrahedra (0, a, a + b, 7) for the six orders (a, b, c) of the axes x = 1, y = 2, z = 4 in lexicographic order.
 * Their edges are the seven kinds +x +y +z +xy +yz +xz +xyz (in this order) per lattice point, the split is the same in every cell, so neighbours
 * agree on shared faces and a closed level set gives a closed mesh.  v < 0 is inside (a NaN is outside).  The mesh is indexed:
 *   a vertex belongs to a lattice edge whose ends differ in sign; vertices are numbered by the exclusive prefix sum of the edge flags in
 *   (voxel linear index, edge kind) order; faces come in (cell linear index, tetrahedron, triangle) order, wound so that the normal points to the
 *   positive values.  With observed_only a cell with a corner of weight 0 emits nothing, and an edge none of whose cells is emitted has no vertex;
 *   a dimension of 1 has no cells.
 * tn_mesh_count writes totals = [vertices, faces] (DEVICE int64[2]) and leaves the flags and the scanned block counts in the workspace;
 * tn_mesh_emit, called with the SAME workspace, volume and observed_only, writes, for the edge from lattice point p = (i, j, k) along e with a = v(p),
 * b = v(p + e), t = a / (a - b):
 *   vertices [V,3] = origin + ((i, j, k) + t e) * voxel;
 *   normals [V,3] = g / |g|, g = g(p) + t (g(p + e) - g(p)), g(q) = the central difference of v at q (one-sided at the volume's border, 0 along an
 *   axis of one point) over the voxel size, |g| = sqrt((gx gx + gy gy) + gz gz); a zero g stays the zero vector;
 *   out_rgbt [V,4] = rgbt of p if t <= 0.5, else of p + e; if that end has weight 0, of the other;
 *   faces [F,3] int32.
 * Rows at or beyond num_vertices / num_faces are not written.  Refused with TN_EINVAL before any launch: dimensions below 1 or 2^31 points and
 * more, null pointers (the outputs may be null when their count is 0), more than 2^31 - 1 vertices, misaligned rgbt arrays, a short workspace.
 *
 * scratch of the two (a flag byte and a first-vertex index per lattice point, two counts and two offsets per block of 256); -1 for refused sizes */
TN_API int64_t tn_mesh_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
TN_API int tn_mesh_count(const float* values, const float* weights, int32_t X, int32_t Y, int32_t Z, int32_t observed_only, int64_t* totals,
                         void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_mesh_emit(const float* values, const float* weights, const float* rgbt, int32_t X, int32_t Y, int32_t Z, int32_t observed_only,
                        float origin_x, float origin_y, float origin_z, float voxel_x, float voxel_y, float voxel_z, float* vertices, float* normals,
                        float* out_rgbt, int64_t num_vertices, int32_t* faces, int64_t num_faces, void* workspace, int64_t workspace_bytes,
                        tn_stream_t stream);

/* ---- Mesh simplification by vertex clustering (where the reference's export runs pymeshlab's quadric edge collapse to a face budget,
 * exporter_utils.py get_mesh_from_filename with target_num_faces; the algorithm here is a different one and no parity with pymeshlab is claimed).
 * The vertices of one cell of a regular grid become one vertex, placed by Lindstrom's quadric rule; faces are remapped, degenerate and duplicate ones
 * dropped.  No atomics: every order comes from a stable sort or a prefix sum, so the same inputs give the same bytes.  The algorithm is stated once,
 * in the header comment of csrc/tn_mesh_simplify.hip; tests/mesh_simplify_functional.py restates it in float64.  In short:
 *   the cell of a vertex is floor((v - origin) / cell) per axis in fp32, clamped to [0, dims - 1]; key = (ix dims_y + iy) dims_z + iz; the clusters
 *   (the vertices of one key) are numbered in key order;
 *   in double and relative to the cell's centre, every input face adds n n^T to A and (n . p0) n to b (n = (p1 - p0) x (p2 - p0)) in the cluster of
 *   each of its corners, in face order; with m the cluster's mean vertex and eps = regularization * trace(A) the new vertex solves
 *   (A + eps I) x = b + eps m, and is m where the trace is 0 or where x leaves the closed cell (by more than 1e-6 cell); rounded to fp32 once;
 *   out_rgbt = the cluster's mean rgbt, out_normals = its normalised normal sum (zero where the sum is zero), both in double, rounded once;
 *   a face with two corners in one cluster is dropped, of the faces that name the same three clusters (in any order) the one with the lowest index
 *   survives, survivors keep their order; clusters no survivor names are not emitted, the others are renumbered in key order.  A face with an index
 *   outside [0, num_vertices) is dropped.
 * vertices [V,3], normals [V,3], rgbt [V,4] (16-byte aligned) fp32, faces [F,3] int32; dims_x dims_y dims_z below 2^31 in all; V <= 2^31 - 1 and
 * 3 F <= 2^31 - 1.  tn_mesh_simplify_count writes to count (DEVICE int64) the number of faces whose corners fall into three different cells -- an upper
 * bound of the simplified mesh's faces, for a search over the cell size: one pass over the vertices and one over the faces, no sort.
 * tn_mesh_simplify_plan writes totals = [vertices, faces] of the simplified mesh (DEVICE int64[2]) and leaves the orders in the workspace;
 * tn_mesh_simplify_emit, called with the SAME workspace, mesh and grid, fills out_vertices / out_normals [num_out_vertices,3], out_rgbt
 * [num_out_vertices,4] and out_faces [num_out_faces,3]; rows at or beyond the two counts are not written.  All three run on the caller's stream
 * without a host synchronisation.  Refused with TN_EINVAL before any launch: sizes outside the above, a grid with a dimension below 1 or 2^31 cells and
 * more, an origin that is not finite, a cell size that is not positive and finite, a negative regularization, null pointers (arrays of 0 rows may be
 * null), misaligned pointers (the workspace to 256 bytes, rgbt arrays to 16), a short workspace.
 *
 * scratch of the three (32 bytes per vertex and 76 per face, and for rocprim's sorts a bound of 36 more per face, or 12 per vertex where that is
 * more, and 1 MiB: the plan checks rocprim's own figures against it and answers TN_ELAUNCH where they do not fit); -1 for refused sizes */
TN_API int64_t tn_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_faces);
TN_API int tn_mesh_simplify_count(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float origin_x, float origin_y,
                                  float origin_z, float cell_x, float cell_y, float cell_z, int32_t dims_x, int32_t dims_y, int32_t dims_z,
                                  int64_t* count, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_mesh_simplify_plan(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float origin_x, float origin_y,
                                 float origin_z, float cell_x, float cell_y, float cell_z, int32_t dims_x, int32_t dims_y, int32_t dims_z,
                                 int64_t* totals, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_mesh_simplify_emit(const float* vertices, const float* normals, const float* rgbt, int64_t num_vertices, const int32_t* faces,
                                 int64_t num_faces, float origin_x, float origin_y, float origin_z, float cell_x, float cell_y, float cell_z,
                                 int32_t dims_x, int32_t dims_y, int32_t dims_z, float regularization, float* out_vertices, float* out_normals,
                                 float* out_rgbt, int64_t num_out_vertices, int32_t* out_faces, int64_t num_out_faces, void* workspace,
                                 int64_t workspace_bytes, tn_stream_t stream);

/* ---- Poisson surface reconstruction from an oriented point cloud (ns-export poisson: nerfstudio/scripts/exporter.py ExportPoissonMesh, Open3D's
 * create_from_point_cloud_poisson).  A dense-grid solve, not Kazhdan's adaptive octree: no parity with Open3D's triangulation is claimed.  The
 * normals are splatted onto a lattice, a Poisson equation is solved on it by conjugate gradients, and tn_mesh_count / tn_mesh_emit extract a level
 * of the solution.  tests/poisson_functional.py restates every rule below in float64.
 *
 * All volumes are [X,Y,Z] fp32, z fastest; lattice point (i, j, k) sits at origin + (i, j, k) * voxel (the volume of the TSDF export).  X, Y and Z are
 * at least 2 and X * Y * Z is below 2^31.  `double` below means: the fp32 inputs widened, every operation rounded on its own (no fused multiply-add).
 *
 * tn_poisson_bin   the plan of a cloud on a grid.  For point p and each axis t = (p - origin) / voxel in double and c = floor(t).  A point is
 *                  skipped when a coordinate (or its t) is not finite or when any c lies outside 0..dim - 2 (a point on the upper outer faces has
 *                  c = dim - 1 and is skipped).  The kept points are ordered by cell key (cx (Y - 1) + cy) (Z - 1) + cz and, inside a cell, by
 *                  ascending point index: rocprim's stable radix sort of (key, index); the first row of every cell is a lower bound over the sorted
 *                  keys.  The plan lives in the workspace and serves any number of tn_poisson_splat calls with the same points and grid.
 * tn_poisson_splat out [X,Y,Z,C] = sum over the kept points of (w_p tri_p(q)) value_p[c], for values [n,C], C in 1..4 (null: all ones, C = 1, the
 *                  density) and weights [n] (null: 1).  A point whose weight or any of whose C values is not finite is skipped.  With f = t - floor(t),
 *                  tri_p(q) = (wx wy) wz in double, w_a = 1 - f_a where q is the lower corner of the point's cell along a and f_a where it is the
 *                  upper one.  A gather: one thread per lattice point walks its eight adjacent cells in lexicographic order of the offset
 *                  (-1 | 0 along x slowest, z fastest) and, inside a cell, the plan's order; it accumulates in double and rounds once to fp32.  No
 *                  atomics: the same inputs give the same bits.  With normalize = 1 the output is sum / den, den = sum of w_p tri_p(q) over the same
 *                  points in the same order, and 0 where den is not positive (RGB+T per lattice point).  n == 0 writes zeros.
 * tn_poisson_sample out [n] DOUBLE = the trilinear interpolation of volume at the points: t as above, c = clamp(floor(t), 0, dim - 2), f = t - c (a
 *                  point outside the grid extrapolates its border cell), the sum over the eight corners in lexicographic order of the offset
 *                  (0 | 1, x slowest) of ((wx wy) wz) value, w_a = 1 - f_a | f_a, in double.  A point with a non-finite t gives NaN.
 * tn_poisson_divergence  out = -div V for V [X,Y,Z,3]: d_a = (V_a(q + e_a) - V_a(q - e_a)) / (2 voxel_a) with V = 0 outside the grid,
 *                  out = -((d_x + d_y) + d_z), in double, rounded once.
 * tn_poisson_apply out = A x: a_a = ((2 x(q) - x(q - e_a)) - x(q + e_a)) / (voxel_a voxel_a) with x = 0 outside the grid (a Dirichlet boundary),
 *                  out = (a_x + a_y) + a_z, plus screening(q) x(q) where screening [X,Y,Z] (non-negative; null: none) is given; in double, rounded
 *                  once.  out must not be x.
 * tn_poisson_solve conjugate gradients on A x = b.  x is in/out and is the starting guess.  x, r, p and A p are stored in fp32; r = b - A x with A x
 *                  rounded as tn_poisson_apply rounds it; every update (x += alpha p, r -= alpha A p, p = r + beta p) is evaluated in double and
 *                  rounded once.  Every dot product is one double partial per block (at most 1024 blocks of 256 threads, grid-stride beyond) folded
 *                  in a fixed order; alpha = r.r / p.Ap and beta = r.r(new) / r.r stay on the device in double.  The run stops after the first
 *                  iteration with r.r <= tol^2 b.b (r the recursive residual; before the first one if the guess already satisfies it) or after
 *                  max_iterations.  The stop is decided on the device: later launches read a flag and return, so the result does not depend on
 *                  check_every.  Three launches per iteration and no host synchronisation inside one; the host reads the state back every
 *                  check_every iterations only, so this call synchronises the stream and cannot be captured into a graph.  record (HOST double[3])
 *                  receives [iterations run, r.r, b.b].  tol = 0 runs exactly max_iterations iterations (unless r.r reaches 0).
 * Refused with TN_EINVAL before any launch: null pointers (values, weights and screening may be null; arrays of 0 points may be), a dimension below
 * 2 or 2^31 lattice points and more, n negative or at or above 2^31, C outside 1..4 (or above 1 without values), normalize other than 0 or 1, an origin
 * that is not finite, a voxel size that is not positive and finite, a negative or non-finite tol, a negative max_iterations, check_every below 1, a
 * workspace that is short or not 256-byte aligned.  n == 0 is TN_OK everywhere.
 *
 * scratch of tn_poisson_bin / tn_poisson_splat (12 bytes per point, 4 per cell, and for rocprim's sort a bound of 12 more per point and 1 MiB:
 * the plan checks rocprim's own figure against it and answers TN_ELAUNCH where it does not fit); 0 for n == 0, -1 for refused sizes */
TN_API int64_t tn_poisson_workspace_bytes(int64_t n, int32_t X, int32_t Y, int32_t Z);
TN_API int tn_poisson_bin(const float* points, int64_t n, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y, float origin_z,
                          float voxel_x, float voxel_y, float voxel_z, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_poisson_splat(const float* points, int64_t n, const float* values, int32_t C, const float* weights, int32_t normalize, int32_t X,
                            int32_t Y, int32_t Z, float origin_x, float origin_y, float origin_z, float voxel_x, float voxel_y, float voxel_z,
                            float* out, const void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_poisson_sample(const float* points, int64_t n, const float* volume, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y,
                             float origin_z, float voxel_x, float voxel_y, float voxel_z, double* out, tn_stream_t stream);
TN_API int tn_poisson_divergence(const float* field, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y, float voxel_z, float* out,
                                 tn_stream_t stream);
TN_API int tn_poisson_apply(const float* x, const float* screening, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y, float voxel_z,
                            float* out, tn_stream_t stream);
/* scratch of tn_poisson_solve (r, p and A p, two rows of block partials, two state slots); -1 for refused sizes */
TN_API int64_t tn_poisson_solve_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
TN_API int tn_poisson_solve(const float* b, const float* screening, float* x, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y,
                            float voxel_z, double tol, int32_t max_iterations, int32_t check_every, double* record, void* workspace,
                            int64_t workspace_bytes, tn_stream_t stream);

/* ---- Texture baking for exported meshes (nerfstudio/exporter/texture_utils.py with unwrap_method "custom": unwrap_mesh_per_uv_triangle, and the ray
 * length and origin offset of export_textured_mesh; xatlas unwrapping is not built).  The atlas, the weights and the kernels are stated once, in the
 * header comment of csrc/tn_texture.hip; tests/texture_functional.py restates the reference's formula.  In short, for F faces and px =
 * px_per_uv_triangle >= 2: two faces share a square of (px + 3) x px texels, squares = ceil(F / 2) in row-major order, squares_w = ceil(sqrt(squares)),
 * squares_h = ceil(squares / squares_w), the image is W = squares_w (px + 3) by H = squares_h px; a texel with the local offsets (i, j) in its square
 * belongs to the lower-right (odd) face iff i + j >= px + 1 and has the weights w1 = i / (px - 1), w2 = j / (px - 1) (upper-left) or
 * w1 = (px + 2 - i) / (px - 1), w2 = (px - 1 - j) / (px - 1) (lower-right), w0 = (1 - w1) - w2, in double -- the reference's barycentric weights,
 * whose corners lie on texel centres, without its float32 cancellation.  A texel whose face index is not below F takes the last face (finite values
 * no texture coordinate addresses).  A face that names a vertex outside [0, num_vertices) gives zeros.  vertices / normals [V,3], rgbt [V,4] (16-byte
 * aligned) fp32, faces [F,3] int32; F in 1..(2^31 - 1) / 3, V in 1..2^31 - 1, px in 2..32768.  Texels are counted row-major, texel = y W + x.
 * Every entry point runs on the caller's stream without a host synchronisation and without atomics: the same inputs give the same bytes.  Refused with
 * TN_EINVAL before any launch: sizes outside the above, a texel range that leaves the image, null or misaligned pointers (outputs of 0 texels may be
 * null), a negative or non-finite raylen, a short workspace.
 *
 * tn_texture_layout     HOST only, no device: layout = [W, H, squares_w, squares_h] (host int64[4])
 * tn_texture_coords     texture_coordinates [F,3,2]: (corner texel + 0.5) / (W, H) in double, rounded once; v counts from the image's top row
 * tn_texture_rays       texels [texel0, texel0 + count): origins [count,3] = sum w_i v_i, directions [count,3] = -sum w_i n_i over max(length, 1e-12)
 *                       (both in double, rounded once; three zero normals give a zero direction), then origins -= (raylen / 2) directions in fp32
 * tn_texture_vertex     the same texels: out_rgbt [count,4] = sum w_i rgbt[v_i], in double, rounded once
 * tn_texture_store      a chunk's rgb (rows of 3 adjacent floats, rgb_stride floats apart) and thermal (thermal_stride apart) into the images of
 *                       num_texels texels at texel0: rgb_image uint8 [num_texels,3] and thermal_image uint8 [num_texels] = rint(255 clamp(v, 0, 1))
 *                       (half to even; a NaN gives 0), and, unless null, float_image [num_texels,4] (16-byte aligned) = the values as they are
 * tn_mesh_mean_edge     mean (DEVICE float) = the mean of |v1 - v0| over the faces (export_textured_mesh's raylen is twice that): norms and sums in
 *                       double, in a fixed order; scratch of tn_mesh_mean_edge_workspace_bytes (8-byte aligned; -1 for refused sizes) */
TN_API int tn_texture_layout(int64_t num_faces, int32_t px_per_uv_triangle, int64_t* layout);
TN_API int tn_texture_coords(int64_t num_faces, int32_t px_per_uv_triangle, float* texture_coordinates, tn_stream_t stream);
TN_API int tn_texture_rays(const float* vertices, const float* normals, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                           int32_t px_per_uv_triangle, float raylen, int64_t texel0, int64_t count, float* origins, float* directions,
                           tn_stream_t stream);
TN_API int tn_texture_vertex(const float* rgbt, int64_t num_vertices, const int32_t* faces, int64_t num_faces, int32_t px_per_uv_triangle,
                             int64_t texel0, int64_t count, float* out_rgbt, tn_stream_t stream);
TN_API int tn_texture_store(const float* rgb, int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t count, int64_t texel0,
                            int64_t num_texels, uint8_t* rgb_image, uint8_t* thermal_image, float* float_image, tn_stream_t stream);
TN_API int64_t tn_mesh_mean_edge_workspace_bytes(int64_t num_faces);
TN_API int tn_mesh_mean_edge(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float* mean, void* workspace,
                             int64_t workspace_bytes, tn_stream_t stream);
/* ---- Frames for people: the reference's colour maps and the side-by-side frame of ns-render (nerfstudio/utils/colormaps.py apply_colormap /
 * apply_float_colormap / apply_depth_colormap, scripts/render.py _render_trajectory_video).  The rule is stated once, in the header comment of
 * csrc/tn_render.hip; tests/render_functional.py restates it in torch.  In short, for a one-channel value x, in fp32 with every operation rounded on
 * its own: depth panels x = clip((x - near) / f32(double(far) - double(near) + 1e-10), 0, 1) with near / far the record's planes where TN_FRAME_NEAR /
 * TN_FRAME_FAR are set and the frame's min / max otherwise; with TN_FRAME_NORMALIZE x = (x - lo) / ((hi - lo) + 1e-9f) over the frame's min / max;
 * x = clip(x f32(colormap_max - colormap_min) + colormap_min, 0, 1); with TN_FRAME_INVERT 1 - x; a NaN becomes 0; the colour is (x, x, x) without a
 * table and row trunc(255 x) of the table [256,3] with one; depth panels with an accumulation a then colour a + (1 - a).  Three-channel panels pass
 * through.  Bytes are trunc(clip(c, 0, 1) 255 + 0.5), a NaN gives 0.  Min and max are over the FINITE values of a frame, (0, 0) where there are none.
 * Every entry point runs on the caller's stream without a host synchronisation and without atomics: the same inputs give the same bytes.  Refused with
 * TN_EINVAL before any launch: null pointers (accumulation and table may be null; minmax only where the panel needs none), a panel count outside
 * 1..TN_FRAME_MAX_PANELS, a channel count other than 1 or 3, sizes below 1 or frames of 2^31 bytes and more, misaligned pointers, a short workspace.
 *
 * tn_frame_minmax   out2 (DEVICE float[2]) = the finite min and max of src [n]: a pair per block and a fixed-order final pass, nothing is read back;
 *                   workspace of TN_FRAME_MINMAX_WORKSPACE_BYTES
 * tn_frame_compose  out_u8 [H, num_panels W, 3]: the panels (HOST array of records, each an [H,W,channels] image) side by side, in one launch; the
 *                   records travel as kernel arguments, their tables are copied to LDS once per block
 * tn_frame_colors   out_rgb [H,W,3] fp32: the colours of one panel before they become bytes (what a viewer takes) */
#define TN_FRAME_MAX_PANELS 8
#define TN_FRAME_MINMAX_WORKSPACE_BYTES 2048
#define TN_FRAME_NORMALIZE 1
#define TN_FRAME_INVERT 2
#define TN_FRAME_DEPTH 4
#define TN_FRAME_NEAR 8  /* near_plane is given (else the frame's min) */
#define TN_FRAME_FAR 16  /* far_plane is given (else the frame's max) */
typedef struct TnFramePanel {
  const float* src;          /* DEVICE [H,W,channels] */
  const float* accumulation; /* DEVICE [H,W] or NULL: depth panels blend over it */
  const float* minmax;       /* DEVICE [2] (tn_frame_minmax of src) or NULL where the panel needs none */
  const float* table;        /* DEVICE [256,3] or NULL (grey) */
  double near_plane, far_plane;       /* doubles, as the reference's Python scalars are: far - near + 1e-10 is taken in double */
  double colormap_min, colormap_max;  /* likewise colormap_max - colormap_min */
  int32_t channels;          /* 1 or 3 */
  int32_t flags;             /* TN_FRAME_* */
} TnFramePanel;
TN_API int tn_frame_minmax(const float* src, int64_t n, float* out2, void* workspace, int64_t workspace_bytes, tn_stream_t stream);
TN_API int tn_frame_compose(const TnFramePanel* panels, int32_t num_panels, int32_t H, int32_t W, uint8_t* out_u8, tn_stream_t stream);
TN_API int tn_frame_colors(const TnFramePanel* panel, int32_t H, int32_t W, float* out_rgb, tn_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* THERMAL_NERF_HIP_H */
