/*
 * mvhmr_unproject.h -- C ABI of the MI355X-native volumetric un-projection ("the hot path").
 *
 * The reference (yohanshin/MultiviewHMR) has no FFI layer: the boundary this library replaces is the
 * plain Python function
 *
 *     unprojection(features, proj_matricies, coord_volumes, aggregation_method='softmax')
 *         models/aggregation.py:20-87, sole call site models/aggregation.py:193
 *
 * and the autograd graph PyTorch builds through it (grid_sampler_2d_backward etc.).  Every entry
 * point below takes plain device pointers, sizes and a HIP stream -- no torch types -- so that any
 * host (ctypes, a torch C++ extension, a C++ trainer) can bind it; INTEGRATION.md shows the
 * reference-side stub.  multiviewhmr_amd/_capi.py is the ctypes binding the Python host side uses.
 *
 * Conventions
 *   - all pointers are DEVICE pointers on the GPU that `stream` belongs to, except the descriptor;
 *   - everything is stream-ordered: no allocation, no host synchronisation, safe to graph-capture;
 *   - scratch memory comes from the caller (mvhmr_unproject_workspace_bytes), 256-byte aligned;
 *   - tensors are dense row-major in the shapes given per function; voxel index
 *     n = (x*vol_y + y)*vol_z + z, i.e. coord_volumes[b].reshape(-1, 3)  (aggregation.py:30);
 *   - return value: MVHMR_OK or an mvhmr_status_t; mvhmr_last_error() gives the reason (thread-local).
 */
#ifndef MVHMR_UNPROJECT_H
#define MVHMR_UNPROJECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVHMR_ABI_VERSION 4   /* 2: MVHMR_LAYOUT_QUAD became column-major (B,V,C/4,Wf,Hf,4).  3: QUAD + AUTO is geometry-gated and needs its
                                 workspace; explicit GATHER with QUAD input is served; MVHMR_BF16 out_dtype; mvhmr_unproject_backward_supported,
                                 mvhmr_triangulate_dlt.  4: MVHMR_LAYOUT_QUAD_LOG2E (ABI history); additive within 4:
                                 mvhmr_unproject_backward_geometry[_workspace_bytes], mvhmr_unproject_backward_geometry_cuboid[_workspace_bytes],
                                 mvhmr_triangulate_dlt_backward, mvhmr_unproject_backward_deterministic[_workspace_bytes],
                                 mvhmr_unproject_backward_cuboid_deterministic[_workspace_bytes], mvhmr_conv1x1_wgrad_deterministic[_workspace_bytes],
                                 the *_masked entry points and their *_masked_workspace_bytes queries (per-sample view masks), the
                                 *_weighted entry points and their *_weighted_workspace_bytes queries (per-view confidence weights), the
                                 *_visible entry points, their *_visible_workspace_bytes queries and mvhmr_unproject_visibility[_cuboid]
                                 (visibility-aware aggregation), the mvhmr_soft_argmax3d_* entry points (volumetric soft-argmax), the
                                 mvhmr_sample_volume_* entry points (trilinear volume sampling at world points), the mvhmr_volume_peaks*
                                 entry points (3-D non-maximum suppression and top-K proposals), the mvhmr_project_volume_* entry points
                                 (ray-marching volumes into camera-view maps) */

typedef enum mvhmr_status_t {
    MVHMR_OK = 0,
    MVHMR_ERR_INVALID_ARGUMENT = 1, /* null pointer, non-positive size, unknown enum (-> ValueError/RuntimeError in Python) */
    MVHMR_ERR_UNSUPPORTED = 2,      /* legal request this build has no kernel for */
    MVHMR_ERR_WORKSPACE = 3,        /* workspace missing, too small or misaligned */
    MVHMR_ERR_LAUNCH = 4            /* hipGetLastError() after a launch was not hipSuccess */
} mvhmr_status_t;

/* aggregation_method of models/aggregation.py:71-85 */
typedef enum mvhmr_agg_t {
    MVHMR_AGG_SOFTMAX = 0, /* sum_v x_v * softmax_v(x)_v  (aggregation.py:77-83) */
    MVHMR_AGG_SUM = 1,     /* aggregation.py:71-72 */
    MVHMR_AGG_MEAN = 2,    /* aggregation.py:73-74 : divides by V, masked views included */
    MVHMR_AGG_MAX = 3      /* aggregation.py:75-76 */
} mvhmr_agg_t;

/* storage type of features / out / grad_out / grad_features.  Coordinates, projection matrices, tap
 * weights, the cross-view softmax and all accumulation are always fp32.  The reference is fp32 only;
 * MVHMR_F16 is this library's storage mode (SURVEY.md 8d "fp16 convention"). */
typedef enum mvhmr_dtype_t {
    MVHMR_F32 = 0,
    MVHMR_F16 = 1,
    MVHMR_BF16 = 2  /* out_dtype only, with fp32 features: the volume (and grad_out) stored as bf16 for a half-precision consumer
                       (models/regressor.py:70-87 under autocast); round to nearest even at the store, NaN stays NaN */
} mvhmr_dtype_t;

/* memory layout of `features` (and of `grad_features`) */
typedef enum mvhmr_layout_t {
    MVHMR_LAYOUT_BVCHW = 0, /* (B,V,C,Hf,Wf) -- the reference's contract (aggregation.py:22-23, :191) */
    MVHMR_LAYOUT_BVHWC = 1, /* (B,V,Hf,Wf,C) -- channels-last, what the gather variant reads; passing it
                               skips the layout pass (e.g. a channels_last 1x1 conv upstream) */
    MVHMR_LAYOUT_QUAD = 2,  /* (B,V,C/4,Wf,Hf,4) fp32 whatever feat_dtype -- column-major "quad-planar": a pixel's 4 channels
                               are 16 contiguous bytes and a pixel COLUMN is one contiguous run, which is what the brick
                               forward stages into LDS (tall narrow tap windows); produced by mvhmr_convert_features and by
                               mvhmr_conv1x1_to_quad.  C % 4 != 0 (round 5): (C + 3) / 4 quads per view, the last one zero-padded
                               by mvhmr_convert_features; brick kernels only (their loops run the whole quads, the last 1 ... 3
                               channels go per voxel).  Forward and backward accept it; the backward then writes
                               grad_features PLANAR (B,V,C,Hf,Wf).  With MVHMR_VARIANT_AUTO the geometry gate decides on the
                               device as for planar input (the gather side converts the copy to channels-last first: C % 4 == 0) */
    MVHMR_LAYOUT_QUAD_LOG2E = 3 /* the same copy with every value multiplied by log2(e), FORWARD ONLY: what the wave-specialised softmax
                               forward stages (3 / 4 views, fp32 volume, launches of >= 256 bricks): its exponentials are then exp2 of
                               a plain difference and ln 2 is folded into the final multiply (<= 2e-7 relative to the unscaled
                               route).  mvhmr_preferred_layout returns it exactly when the forward accepts it; the backward and every
                               other shape / aggregate answer MVHMR_ERR_UNSUPPORTED.  A forward on planar input makes this copy itself */
} mvhmr_layout_t;

/* kernel selection; AUTO picks the fastest applicable one.  The others exist for tests and profiling.
 * AUTO with planar or quad-planar features of a shape both variants serve decides ON THE DEVICE (cameras and voxel pitch decide whether
 * the brick variant's LDS windows fit): both variants are launched behind a gate and one of them runs; stream-ordered, no
 * host synchronisation.  mvhmr_unproject_selected_variant reports the variant AUTO prefers for the shape. */
typedef enum mvhmr_variant_t {
    MVHMR_VARIANT_AUTO = 0,
    MVHMR_VARIANT_GATHER = 1, /* channel-per-lane gather from L2, any shape */
    MVHMR_VARIANT_BRICK = 2   /* voxel bricks with LDS-staged feature windows (forward) and LDS-accumulated
                                 gradient windows (backward): C % 4 == 0, 1 ... 8 views (1, 3 and 5 / 6 / 7 views run the 2-, 4- and 8-view
                                 kernels with the missing views absent), any volume extents (forward bricks of
                                 4 x 8 x 32 voxels, 8 x 8 x 32 for 2 / 4 views when vol_x > 4; backward 8 x 8 x 16 -- 8 x 4 x 16 with
                                 8 views -- or 4 x 8 x 32 / 4 x 4 x 32, whichever covers the volume with fewer idle lanes; the lanes
                                 of a brick that lie past the volume's edge idle; 16-bit volumes need vol_z even in the forward);
                                 every storage pairing check_desc admits (fp32 / fp16 features with an fp32, fp16 or -- fp32 features -- bf16 volume);
                                 anything else is MVHMR_ERR_UNSUPPORTED.
                                 What therefore runs the GATHER family under AUTO: more than 8 views; C % 4 != 0;
                                 channels-last input; forward launches of fewer than 96 bricks' worth of voxels (B * X * Y * Z <
                                 196 608: one round of bricks costs the same however few they are -- the reference's shipped
                                 16^3 volume, cfg/defaults.py:25, up to batch 47 per GPU); and any call whose cameras / voxel
                                 pitch make the LDS windows overflow (decided on the device).  Its backward is the plane kernel (no
                                 global atomics, 64-bit sums where many taps meet in a pixel) for planar / quad-planar features whose
                                 maps fit LDS, the per-tap float scatter otherwise; AUTO also prefers the plane kernel to bricks when
                                 the volume has fewer bricks than the chip has CUs */
} mvhmr_variant_t;

typedef struct mvhmr_unproject_desc {
    int32_t abi_version; /* MVHMR_ABI_VERSION */
    int32_t batch;       /* B  = features.shape[0]              */
    int32_t views;       /* V  = features.shape[1]   (1..16)    */
    int32_t channels;    /* C  = features.shape[2]              */
    int32_t feat_h;      /* Hf = features.shape[3]              */
    int32_t feat_w;      /* Wf = features.shape[4]              */
    int32_t vol_x;       /* coord_volumes.shape[1]              */
    int32_t vol_y;       /* coord_volumes.shape[2]              */
    int32_t vol_z;       /* coord_volumes.shape[3]              */
    int32_t method;      /* mvhmr_agg_t                         */
    int32_t feat_dtype;  /* mvhmr_dtype_t of features / grad_features */
    int32_t out_dtype;   /* mvhmr_dtype_t of out / grad_out (the reference always returns fp32, aggregation.py:25) */
    int32_t feat_layout; /* mvhmr_layout_t                      */
    int32_t variant;     /* mvhmr_variant_t                     */
} mvhmr_unproject_desc;

/* Name of the kernel family the forward launches for this descriptor ("k_fwd_ws", "k_fwd_brick", "k_fwd_brick_groups", "k_fwd_gather";
 * for MVHMR_VARIANT_AUTO on gated shapes: the brick-side kernel the device-side gate may select): lets a profiler harness match
 * rocprofv3 kernel names without knowing the dispatch rules.  Static storage; NULL for an invalid descriptor. */
const char *mvhmr_unproject_forward_kernel_name(const mvhmr_unproject_desc *desc);

/* 1 when mvhmr_unproject_backward[_cuboid] serves this descriptor (layout x variant x shape), else 0: lets set-up code choose a
 * route before any tensor exists (the forward's counterpart is mvhmr_unproject_selected_variant > 0). */
int mvhmr_unproject_backward_supported(const mvhmr_unproject_desc *desc);

/* Bytes of device scratch forward / backward need for this problem (0 is possible).  Forward: at most one fp32 copy of the features.
 * Backward: a feature copy + an fp32 gradient accumulator of the same size on the brick route; on the coarse-grid (plane) route a tap
 * table and one slab of the Jacobian stream (V x the slab's share of grad_out in fp32, at most ~256 MB: 0.27 GB for BASELINE configs[1]) --
 * ask, do not guess. */
size_t mvhmr_unproject_forward_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_workspace_bytes(const mvhmr_unproject_desc *desc);

/*
 * Forward: replaces unprojection() (models/aggregation.py:20-87).
 *   features  (B,V,C,Hf,Wf) or (B,V,Hf,Wf,C) per desc->feat_layout, desc->feat_dtype   [read]
 *   proj      (B,V,3,4) fp32   -- proj_matricies (aggregation.py:132-133)              [read]
 *   coords    (B,X,Y,Z,3) fp32 -- coord_volumes  (aggregation.py:136,187)              [read]
 *   out       (B,C,X,Y,Z) desc->out_dtype, every element is written                     [write]
 */
int mvhmr_unproject_forward(const mvhmr_unproject_desc *desc, const void *features, const float *proj,
                            const float *coords, void *out, void *workspace, size_t workspace_bytes,
                            void *hip_stream);

/*
 * Backward w.r.t. features: replaces autograd through the reference graph (CopySlices, softmax/mul/sum,
 * masked fill, grid_sampler_2d_backward per (b, v)).  The gradients w.r.t. proj and coords, which the reference's graph
 * also has (a caller that refines cameras or predicts where the volume sits), are mvhmr_unproject_backward_geometry below.
 *   grad_out       (B,C,X,Y,Z) desc->out_dtype                                          [read]
 *   grad_features  same shape/layout/dtype as features, every element is written        [write]
 * Scatter-adds use fp32 float atomics, so low-order bits can differ from run to run.  The brick variant sums a
 * brick's contributions per pixel in fixed point first (one power-of-two scale per channel, resolution ~2^-25 of the
 * channel's largest contribution in the brick) and issues one float atomic per window pixel.
 * Non-finite values: an Inf / NaN in grad_out (or an overflowing product) makes grad_features non-finite.  The gather variant
 * propagates it tap by tap like the reference's float scatter; the brick variant writes NaN to every pixel of the affected
 * brick's tap windows for that channel (a superset of the reference's pixels) -- isfinite(grad) agrees, the exact set differs.
 * Forward: a tap outside the image contributes 0 * (clamped border pixel) instead of being skipped.  With a NON-FINITE feature
 * value in a border pixel the same samples come out non-finite as with grid_sample's zero padding (such a sample also taps the
 * border pixel itself), but an Inf may read NaN; finite outputs are never affected.  A NaN depth (NaN in proj / coords) gives
 * an exactly zero sample for that view.
 */
int mvhmr_unproject_backward(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,
                             const float *proj, const float *coords, void *grad_features, void *workspace,
                             size_t workspace_bytes, void *hip_stream);

/*
 * Backward w.r.t. the geometry: the gradients autograd through the reference graph gives proj_matricies and coord_volumes
 * (grid_sampler_2d_backward's grid gradient, back through the normalisation, the perspective divide and the projection).
 *   grad_out     (B,C,X,Y,Z) desc->out_dtype                                                  [read]
 *   features     as for mvhmr_unproject_backward: BVCHW, BVHWC or QUAD (C % 4 == 0);
 *                MVHMR_LAYOUT_QUAD_LOG2E is MVHMR_ERR_UNSUPPORTED (forward only)                [read]
 *   grad_proj    (B,V,3,4) fp32 or NULL, every element written                                [write]
 *   grad_coords  (B,X,Y,Z,3) fp32 or NULL, every element written                              [write]
 * At least one output must be non-null (both NULL: MVHMR_ERR_INVALID_ARGUMENT).  Any storage pairing check_desc admits, 1 ... 16
 * views, any C and volume extents.  desc->variant is ignored: one kernel family serves every shape.  A view with depth <= 0 takes no
 * part (its gradients are 0); the taps are grid_sampler_2d_backward's, floor() on exact cell boundaries, ix == -1 included.
 * No float atomics: grad_coords is written once per voxel, grad_proj is summed per (sample, view) from fixed-order fp32 partials in
 * float64 -- both are bitwise reproducible from run to run.  The workspace (mvhmr_unproject_backward_geometry_workspace_bytes) holds
 * a channels-last copy of the features (none for MVHMR_LAYOUT_BVHWC) and the partials of grad_proj.
 */
size_t mvhmr_unproject_backward_geometry_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_backward_geometry(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                      const float *coords, float *grad_proj, float *grad_coords, void *workspace, size_t workspace_bytes,
                                      void *hip_stream);

/*
 * The same two calls for the volumes VolumeGenerator.forward builds (models/aggregation.py:138-187): instead of reading a
 * (B,X,Y,Z,3) coordinate tensor the kernels evaluate the reference's recipe per voxel,
 *     coords[b,i,j,k] = rot[b] @ (position + sides / (S - 1) * (i,j,k) - center[b]) + center[b],      S = (vol_x, vol_y, vol_z)
 * with the rounding order of mvhmr_build_coord_volumes, so that both routes are bit-equal.  13 floats per sample replace the
 * coordinate tensor (403 MB per GPU at BASELINE configs[4]) and the kernel that builds it.
 *   rot       (B,9) fp32 row-major, device   -- utils/volumetric.py:87-114 (identity at eval)
 *   center    (B,3) fp32, device             -- the rotation pivot, aggregation.py:180-186
 *   position, sides   3 doubles each, HOST   -- cuboid corner and edge lengths, aggregation.py:143-144
 */
int mvhmr_unproject_forward_cuboid(const mvhmr_unproject_desc *desc, const void *features, const float *proj,
                                   const float *rot, const float *center, const double position[3],
                                   const double sides[3], void *out, void *workspace, size_t workspace_bytes,
                                   void *hip_stream);
int mvhmr_unproject_backward_cuboid(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,
                                    const float *proj, const float *rot, const float *center,
                                    const double position[3], const double sides[3], void *grad_features,
                                    void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Deterministic mode of the two feature-gradient backwards above: the same arguments, validation and error codes, and grad_features
 * bitwise identical from run to run on the same inputs, device and batch layout (no float atomics; nothing sums across samples, so
 * permuting the batch permutes the result).  The kernels follow the default's route, without the geometry gate: the brick kernels
 * (their window sums flushed as int64 fixed point with u64 atomics), the plane kernels (already atomic-free), or the gather kernels (taps
 * added as int64 fixed point).  A scale pass first fixes one power-of-two scale per (sample, channel) from max |grad_out| (and, for
 * softmax, max |features|) so that no sum can overflow; a conversion pass writes grad_features.  A (sample, channel) whose scale bound is not finite gets NaN over its whole gradient: wherever the
 * default route is non-finite this one is too.  Quad-planar features that neither the deterministic brick route (one sample's int64
 * accumulator below 2 GB) nor the plane route takes need C <= 4092 and B * V <= 65535 (the gather route's channels-last conversion),
 * else MVHMR_ERR_UNSUPPORTED.  The workspace
 * (mvhmr_unproject_backward_deterministic_workspace_bytes, at least the default's) holds the feature copy, the int64 accumulator and
 * the scales.
 */
size_t mvhmr_unproject_backward_deterministic_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_backward_deterministic(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                           const float *coords, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,
                                                  const float *proj, const float *rot, const float *center, const double position[3],
                                                  const double sides[3], void *grad_features, void *workspace, size_t workspace_bytes,
                                                  void *hip_stream);

/*
 * Backward w.r.t. the geometry of the cuboid recipe: grad_proj as mvhmr_unproject_backward_geometry gives it (the same partials, the
 * same bits as that call on the coordinates mvhmr_build_coord_volumes builds), and the gradients w.r.t. the pose the recipe takes,
 *   grad_rot     (B,3,3) fp32 or NULL    grad_rot[b][r][k] = sum_n gX_n[r] d_n[k],   d_n = fl(grid_n - center[b])          [write]
 *   grad_center  (B,3) fp32 or NULL      grad_center[b] = sum_n gX_n - rot[b]^T sum_n gX_n                                   [write]
 * with gX_n the gradient w.r.t. the centre of voxel n (dX/dcenter = I - rot).  rot = I gives grad_center == 0 exactly.  Validation,
 * layouts and storage pairings as mvhmr_unproject_backward_geometry; at least one output non-null.  Per-block fp32 partials summed
 * per sample in float64 in a fixed order, no float atomics: bitwise reproducible.  The workspace
 * (mvhmr_unproject_backward_geometry_cuboid_workspace_bytes) holds the channels-last copy when one is needed and the partials of
 * grad_proj and of the pose.
 */
size_t mvhmr_unproject_backward_geometry_cuboid_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_backward_geometry_cuboid(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                             const float *rot, const float *center, const double position[3], const double sides[3],
                                             float *grad_proj, float *grad_rot, float *grad_center, void *workspace, size_t workspace_bytes,
                                             void *hip_stream);

/*
 * Per-sample view masks (additive within ABI 4): the same calls for a batch whose samples do not all have the same cameras.
 *   view_mask  (B,V) uint8, DEVICE, row-major: nonzero = the view is present.  NULL = every view present: the call is then exactly the
 *              unmasked entry point of the same name (same kernels, same bits, same workspace).
 * Sample b with present views P_b (n_b = |P_b|) gets what the unmasked call gives for features[b, P_b], proj[b, P_b] alone: mean divides
 * by n_b, softmax and max range over P_b.  The masked views' features and projection rows are never read (any bits, NaN / Inf included,
 * give the same result); their gradients (grad_features, grad_proj rows) are written as exact zeros.  A sample with n_b = 0 gets a zero
 * volume and zero gradients.  The per-voxel rule (z <= 0 or outside the map: the sample is 0 and still counted) is unchanged.
 * How: a table kernel packs every sample's present views into view slots 0 .. n_b - 1 (increasing view order) and a copy of the
 * features and projections is made in that order; the GATHER kernel family (forward, per-tap scatter backward and its deterministic form)
 * and the geometry kernels then take n_b per sample; gradients are unpacked back into view order.  Stream-ordered, no host
 * synchronisation, graph-capturable; the deterministic and geometry forms keep their bitwise reproducibility.
 * Limits: features in MVHMR_LAYOUT_BVCHW or MVHMR_LAYOUT_BVHWC -- MVHMR_LAYOUT_QUAD / _QUAD_LOG2E with a non-null mask is
 * MVHMR_ERR_UNSUPPORTED (hand over the planar features); desc->variant AUTO or GATHER (MVHMR_VARIANT_BRICK with a mask is
 * MVHMR_ERR_UNSUPPORTED: the brick kernels, the plane backward and the wave-specialised forward take no per-sample view count yet).
 * An all-true mask therefore reproduces the unmasked call with MVHMR_VARIANT_GATHER bit for bit where that call's backward is the
 * per-tap scatter (channels-last features, or maps too large for the plane kernel), and within the variants' tolerance elsewhere.
 * Workspace: the *_masked_workspace_bytes queries (a table, one or two packed copies of the features / gradient, and the gather route's
 * own workspace; never less than the unmasked call needs, so a NULL mask is served by the same buffer).  Storage pairings, 1 ... 16 views
 * and every other validation as the unmasked calls.
 */
size_t mvhmr_unproject_forward_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_masked_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_masked(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords,
                                   const uint8_t *view_mask, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_masked(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot,
                                          const float *center, const double position[3], const double sides[3], const uint8_t *view_mask,
                                          void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                    const float *coords, const uint8_t *view_mask, void *grad_features, void *workspace, size_t workspace_bytes,
                                    void *hip_stream);
int mvhmr_unproject_backward_cuboid_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                           const float *rot, const float *center, const double position[3], const double sides[3],
                                           const uint8_t *view_mask, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                  const float *coords, const uint8_t *view_mask, void *grad_features, void *workspace,
                                                  size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,
                                                         const float *proj, const float *rot, const float *center, const double position[3],
                                                         const double sides[3], const uint8_t *view_mask, void *grad_features, void *workspace,
                                                         size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                             const float *coords, const uint8_t *view_mask, float *grad_proj, float *grad_coords, void *workspace,
                                             size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_masked(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                    const float *rot, const float *center, const double position[3], const double sides[3],
                                                    const uint8_t *view_mask, float *grad_proj, float *grad_rot, float *grad_center, void *workspace,
                                                    size_t workspace_bytes, void *hip_stream);

/*
 * Per-view confidence weights (additive within ABI 4): the *_masked calls with one more argument beside view_mask.
 *   view_weights  (B,V) fp32, DEVICE, row-major.  NULL = unweighted: the call is then exactly the *_masked entry point of the same name
 *                 (same kernels, same bits, same workspace need).  view_mask may be NULL as well (every view the weights leave present).
 * Per sample b the present views are P_b = { v : (no mask or view_mask[b,v] != 0) and view_weights[b,v] > 0 }: a weight that is zero,
 * negative or NaN means ABSENT in the view masks' sense -- features and projection row never read, grad_features, grad_proj row and
 * grad_weights entry written as exact zeros.  The values are not inspected on the host; nothing synchronises.  With s_v the per-view
 * sample of a voxel and channel (zero where z <= 0 or the taps leave the map; such zeros take part) and W = sum_{P_b} w_v:
 *     sum      out = sum_P w_v s_v                                          d out / d w_v = s_v
 *     mean     out = sum_P w_v s_v / W                                      d out / d w_v = (s_v - out) / W
 *     softmax  out = sum_P p_v s_v,  p_v = w_v e^{s_v} / sum_P w_u e^{s_u}   d out / d w_v = (p_v / w_v) (s_v - out)
 *     max      MVHMR_ERR_UNSUPPORTED with non-null weights (no weighted form)
 * all in fp32.  P_b empty: a zero volume and zero gradients.  Weights in {0, 1} are the view_mask call, all ones the unweighted one, an
 * integer weight k the unweighted call on a sample that holds the view k times; mean and softmax do not change when a sample's weights
 * are multiplied by one positive constant.
 * The two geometry calls gain grad_weights (B,V) fp32 (nullable; every element written): the sum over the sample's voxels and channels
 * of grad_out times the derivative above, as fp32 partials per block in a fixed order summed in float64 -- bitwise reproducible like
 * grad_proj.  It may be the only output asked for; all outputs null is MVHMR_ERR_INVALID_ARGUMENT, and so is grad_weights without
 * view_weights.  The deterministic backward bounds its fixed-point scale with the weights (sum: max |grad_out| times the sample's largest
 * weight).  Limits, layouts, storage pairings, variants (quad-planar layouts and MVHMR_VARIANT_BRICK refused) as the masked calls.
 * Workspace: the *_weighted_workspace_bytes queries, never less than the masked ones.
 */
size_t mvhmr_unproject_forward_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_weighted_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_weighted(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords,
                                     const uint8_t *view_mask, const float *view_weights, void *out, void *workspace, size_t workspace_bytes,
                                     void *hip_stream);
int mvhmr_unproject_forward_cuboid_weighted(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot,
                                            const float *center, const double position[3], const double sides[3], const uint8_t *view_mask,
                                            const float *view_weights, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                      const float *coords, const uint8_t *view_mask, const float *view_weights, void *grad_features, void *workspace,
                                      size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                             const float *rot, const float *center, const double position[3], const double sides[3],
                                             const uint8_t *view_mask, const float *view_weights, void *grad_features, void *workspace,
                                             size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                    const float *coords, const uint8_t *view_mask, const float *view_weights, void *grad_features,
                                                    void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,
                                                           const float *proj, const float *rot, const float *center, const double position[3],
                                                           const double sides[3], const uint8_t *view_mask, const float *view_weights,
                                                           void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                               const float *coords, const uint8_t *view_mask, const float *view_weights, float *grad_proj,
                                               float *grad_coords, float *grad_weights, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_weighted(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                      const float *rot, const float *center, const double position[3], const double sides[3],
                                                      const uint8_t *view_mask, const float *view_weights, float *grad_proj, float *grad_rot,
                                                      float *grad_center, float *grad_weights, void *workspace, size_t workspace_bytes,
                                                      void *hip_stream);

/*
 * Visibility-aware aggregation (additive within ABI 4): the *_visible entry points are the *_masked ones -- same arguments,
 * view_mask (B,V) uint8 on the DEVICE and nullable (NULL = every view present) -- with every VOXEL aggregating only the views that see it.
 * With ix, iy, z the fp32 pixel position and depth the kernels compute for (voxel n, view v), view v SEES n iff
 *     z > 0  and  0 <= ix <= Wf - 1  and  0 <= iy <= Hf - 1
 * both ends inclusive; NaN anywhere, or z == 0, is not seen.  A seen view's bilinear footprint lies wholly inside the map; a view whose
 * footprint is only partly inside (-1 < ix < 0 ...) is NOT seen, although the plain call gives it a non-zero sample.  S(b,n) = the
 * present views that see n; with s_v the per-view sample:
 *     sum      out = sum_S s_v                 mean  out = sum_S s_v / |S|
 *     max      out = max_S s_v                 softmax  out = sum_S p_v s_v, p the softmax over S
 * |S| = 0 gives out = 0 and exact-zero gradients for that voxel; a view outside S is not read for that voxel (non-finite feature values
 * only unseen voxel-views would tap never reach the output) and receives exact zeros.  S is piecewise constant in the geometry, so the
 * geometry gradients are the plain call's chain rule restricted to v in S.  The deterministic backward bounds the mean's fixed-point scale
 * by max |grad_out| alone (a voxel may be seen by one view).  Limits, layouts, storage pairings, variants (quad-planar layouts and
 * MVHMR_VARIANT_BRICK refused with MVHMR_ERR_UNSUPPORTED; AUTO runs the gather family) as the masked calls.  No view_weights yet.
 * Workspace: the *_visible_workspace_bytes queries, never less than the masked ones; without a mask nothing is packed or copied.
 *
 * mvhmr_unproject_visibility[_cuboid] writes the sets themselves: bits (B,X,Y,Z) int32 on the device, bit v set iff view v is present
 * (view_mask nullable) and sees the voxel.  desc->channels, dtypes and method are not used; no workspace; one kernel on hip_stream.
 */
size_t mvhmr_unproject_forward_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_visible_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_visible(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords, const uint8_t
                                    *view_mask, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_visible(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot, const float
                                           *center, const double position[3], const double sides[3], const uint8_t *view_mask, void *out, void
                                           *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float
                                     *coords, const uint8_t *view_mask, void *grad_features, void *workspace, size_t workspace_bytes, void
                                     *hip_stream);
int mvhmr_unproject_backward_cuboid_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const
                                            float *rot, const float *center, const double position[3], const double sides[3], const uint8_t
                                            *view_mask, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                   const float *coords, const uint8_t *view_mask, void *grad_features, void *workspace, size_t
                                                   workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float
                                                          *proj, const float *rot, const float *center, const double position[3], const double
                                                          sides[3], const uint8_t *view_mask, void *grad_features, void *workspace, size_t
                                                          workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const
                                              float *coords, const uint8_t *view_mask, float *grad_proj, float *grad_coords, void *workspace, size_t
                                              workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_visible(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                     const float *rot, const float *center, const double position[3], const double sides[3], const
                                                     uint8_t *view_mask, float *grad_proj, float *grad_rot, float *grad_center, void *workspace,
                                                     size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_visibility(const mvhmr_unproject_desc *desc, const float *proj, const float *coords, const uint8_t *view_mask, int32_t *bits, void
                               *hip_stream);
int mvhmr_unproject_visibility_cuboid(const mvhmr_unproject_desc *desc, const float *proj, const float *rot, const float *center, const double
                                      position[3], const double sides[3], const uint8_t *view_mask, int32_t *bits, void *hip_stream);

/*
 * Cross-view variance (additive within ABI 4): the *_moments entry points are the *_visible ones with two arguments behind
 * `view_mask` (nullable as there): `visible` (0: every present view takes part, a view behind the camera or outside the map with its sample
 * of zero, as in the plain mean; non-zero: the present views that see the voxel, the seeing test of the *_visible calls) and `moments`.
 * With S the participating views of one (voxel, channel), n = |S| and s_v the per-view samples, in fp32 and in view order:
 *     mu  = (sum_S s_v) / n                 var = (sum_S (s_v - mu)^2) / n       (population variance around the ROUNDED mu)
 * var >= 0, var = 0 exactly for n = 1, mu = var = 0 for n = 0 (exact-zero gradients there).  MVHMR_MOMENTS_VAR: out / grad_out hold C
 * channels, the variance.  MVHMR_MOMENTS_MEANVAR: 2C channels, [0, C) the mean -- the bits of the *_visible / *_masked mean call with the
 * gather variant -- and [C, 2C) the variance -- the bits of MVHMR_MOMENTS_VAR.  Any other value is MVHMR_ERR_INVALID_ARGUMENT.
 * desc->method names the moment the variance is taken around and must be MVHMR_AGG_MEAN (anything else: MVHMR_ERR_UNSUPPORTED).
 * Gradient: ds_v = (2 g_v / n) (s_v - mu) + g_m / n for v in S with g_m, g_v the halves of grad_out (g_m = 0 for MVHMR_MOMENTS_VAR), exactly 0
 * outside S; the geometry gradients are the existing chain rule driven by these.  The deterministic backward bounds its fixed-point scale
 * by max |g_m| + 4 max |g_v| Fmax per (b, c), Fmax the largest |feature| a participating view taps.  Limits, layouts, storage pairings,
 * variants (quad-planar layouts and MVHMR_VARIANT_BRICK refused with MVHMR_ERR_UNSUPPORTED; AUTO runs the gather family) as the visible calls.
 * Workspace: the *_moments_workspace_bytes queries, never less than the visible ones; without a mask nothing is packed or copied.
 */
typedef enum mvhmr_moments_t {
    MVHMR_MOMENTS_VAR = 1,
    MVHMR_MOMENTS_MEANVAR = 2
} mvhmr_moments_t;
size_t mvhmr_unproject_forward_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_moments_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_moments(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords, const uint8_t *view_mask, int32_t visible, int32_t moments, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_moments(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot, const float
                                           *center, const double position[3], const double sides[3], const uint8_t *view_mask, int32_t visible, int32_t moments, void *out, void
                                           *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float
                                     *coords, const uint8_t *view_mask, int32_t visible, int32_t moments, void *grad_features, void *workspace, size_t workspace_bytes, void
                                     *hip_stream);
int mvhmr_unproject_backward_cuboid_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const
                                            float *rot, const float *center, const double position[3], const double sides[3], const uint8_t *view_mask, int32_t visible, int32_t moments, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                   const float *coords, const uint8_t *view_mask, int32_t visible, int32_t moments, void *grad_features, void *workspace, size_t
                                                   workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float
                                                          *proj, const float *rot, const float *center, const double position[3], const double
                                                          sides[3], const uint8_t *view_mask, int32_t visible, int32_t moments, void *grad_features, void *workspace, size_t
                                                          workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const
                                              float *coords, const uint8_t *view_mask, int32_t visible, int32_t moments, float *grad_proj, float *grad_coords, void *workspace, size_t
                                              workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_moments(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
                                                     const float *rot, const float *center, const double position[3], const double sides[3], const uint8_t *view_mask, int32_t visible, int32_t moments, float *grad_proj, float *grad_rot, float *grad_center, void *workspace,
                                                     size_t workspace_bytes, void *hip_stream);

/*
 * Per-pixel view confidence maps: the *_confidence entry points are the *_visible ones with `view_confidence` behind
 * `view_mask` and the seeing test as the flag `visible` (0: off).  view_confidence (B,V,Hf,Wf) fp32 planar on the device: one map per view at
 * feature resolution, or NULL -- then the call is exactly the masked call (visible == 0) or the visible call (visible != 0).
 *
 * For voxel n of sample b and view v take ix, iy, z, the four taps and their weights exactly as the features' sample s_v does (same rounding
 * order, quirk Q1, zero padding).  c_v is the map of (b, v) sampled with the same taps and weights by the same fused multiply-adds: one more
 * channel.  Present set S(b, n) = { v : view_mask[b][v] != 0 (if given) and c_v > 0 [and view v sees the voxel, if visible] }.  The test is
 * c_v > 0: a sample that is zero, negative or NaN makes the view absent for that voxel, and so does z <= 0 or a footprint wholly outside the
 * map (c_v = 0 there: quirk Q2 does not apply to a confidence call).  An absent view's features are not read for that voxel and it receives
 * exact-zero gradients.  With W = sum_S c_v, everything in fp32:
 *     method    out                                        ds_v (v in S)              dc_v (v in S), per channel
 *     sum       sum_S c_v s_v                              g c_v                      g s_v
 *     mean      sum_S c_v s_v / W                          g c_v / W                  g (s_v - out) / W
 *     softmax   sum_S p_v s_v,                             g p_v (1 + s_v - out)      g (p_v / c_v) (s_v - out)
 *               p_v = c_v e^(s_v - m) / sum_S c_u e^(s_u - m), m = max_S s
 *     max       refused: MVHMR_ERR_UNSUPPORTED, as for view_weights
 * An empty S gives out = 0 and exact-zero gradients for that voxel.  Per-view scalar weights are the case of a constant map, a mask the case
 * of an all-zero map; mean and softmax do not change when all maps of a sample are scaled by one positive constant.
 *
 * Gradients.  grad_features: the four taps times ds_v.  The geometry calls gain grad_confidence (B,V,Hf,Wf) fp32 [write]: for every voxel the
 * sum over channels of dc_v, scattered to the map by the same four tap weights; nullable, every element written when given (zeros for views a
 * mask drops), it may be the only output, all outputs null is MVHMR_ERR_INVALID_ARGUMENT, and grad_confidence without view_confidence is
 * MVHMR_ERR_INVALID_ARGUMENT.  It is bitwise reproducible in every mode (fixed-order sums, then int64 fixed point with one power-of-two
 * exponent per (b, v) taken from the measured largest |sum_channels dc_v|; a (b, v) whose largest value is not finite comes back NaN).
 * grad_proj, grad_coords, grad_rot, grad_center: the plain call's chain rule over v in S (S is piecewise constant; out is continuous where
 * c_v -> 0+) with one more term per view, (sum_channels dc_v) * grad c_v(ix, iy), the confidence sample's own position derivative.
 * The deterministic feature backward bounds the sum's fixed-point scale by max |grad_out| times the sample's largest confidence pixel, the
 * mean's and the softmax's as the visible calls do.
 * Limits, layouts, storage pairings, variants as the masked calls: quad-planar layouts and MVHMR_VARIANT_BRICK are refused with
 * MVHMR_ERR_UNSUPPORTED, AUTO runs the gather family.  Workspace: the *_confidence_workspace_bytes queries, never less than the masked or
 * visible ones; without a mask nothing is packed or copied, with one the maps are packed in slot order together with the features.
 */
size_t mvhmr_unproject_forward_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_confidence_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_confidence(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords,
        const uint8_t *view_mask, const float *view_confidence, int visible, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *coords,
        const uint8_t *view_mask, const float *view_confidence, int visible, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *coords,
        const uint8_t *view_mask, const float *view_confidence, int visible, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *coords,
        const uint8_t *view_mask, const float *view_confidence, int visible, float *grad_proj, float *grad_coords, float *grad_confidence, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_confidence(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot, const float *center, const double position[3], const double sides[3],
        const uint8_t *view_mask, const float *view_confidence, int visible, void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *rot, const float *center, const double position[3], const double sides[3],
        const uint8_t *view_mask, const float *view_confidence, int visible, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *rot, const float *center, const double position[3], const double sides[3],
        const uint8_t *view_mask, const float *view_confidence, int visible, void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_confidence(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *rot, const float *center, const double position[3], const double sides[3],
        const uint8_t *view_mask, const float *view_confidence, int visible, float *grad_proj, float *grad_rot, float *grad_center, float *grad_confidence, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Shared feature maps (additive within ABI 4): `volumes` (M) volumes are un-projected from the desc->batch (B) feature
 * samples through feature_index, M int32 on the device.  Volume m is the plain un-projection of features[feature_index[m]] under
 * proj[feature_index[m]] onto coords[m] (tensor form: coords (M,X,Y,Z,3)) or the cuboid of rot[m], center[m] (cuboid form: rot (M,3,3),
 * center (M,3); position and sides shared).  The index may repeat a sample, skip one and come in any order.  The descriptor keeps its
 * meaning: desc->batch is B, the number of FEATURE samples; features and proj are (B, ...), out and grad_out are (M,C,X,Y,Z).
 *   grad_features (B, ...): sample b receives the sum over the volumes that name it; every element is written, a sample no volume names
 *       gets exact zeros.  Deterministic form: one exponent per feature sample and channel, whose bound counts the volumes that name it.
 *   grad_proj (B,V,3,4): summed over the same volumes, float64, volumes in ascending order then their blocks in order (bitwise
 *       reproducible); a sample no volume names gets zeros.  grad_coords (M,X,Y,Z,3), grad_rot (M,3,3), grad_center (M,3): per volume.
 * An entry outside [0, B) is "no sample": that volume is exact zeros, contributes to no gradient (its own geometry gradients are zeros),
 * and nothing is read through it.  Nothing is inspected on the host: no synchronisation, the calls stay graph-capturable.
 * Routing and refusals are those of the *_masked calls: the gather kernels (MVHMR_VARIANT_AUTO runs them), planar or channels-last
 * features; MVHMR_VARIANT_BRICK and the quad-planar layouts -> MVHMR_ERR_UNSUPPORTED.  1 <= volumes (MVHMR_ERR_INVALID_ARGUMENT) <= 65535
 * (MVHMR_ERR_UNSUPPORTED: the volume index is the grid's y extent).  A null feature_index needs volumes == batch
 * (MVHMR_ERR_INVALID_ARGUMENT) and is the plain call with MVHMR_VARIANT_GATHER.  view_mask, view_weights, view_confidence and visible are
 * the view selections of the families above; they do not compose with the index yet: each must be null / 0, else MVHMR_ERR_UNSUPPORTED with
 * its own text.
 * Workspace: the *_shared_workspace_bytes queries take `volumes` too.  Every feature-sized region (channels-last copy, gradient
 * accumulator) is sized by B; only the geometry calls' partials grow with M.  Each total also covers the plain call's.
 */
size_t mvhmr_unproject_forward_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_forward_cuboid_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_cuboid_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_deterministic_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_cuboid_deterministic_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_geometry_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
size_t mvhmr_unproject_backward_geometry_cuboid_shared_workspace_bytes(const mvhmr_unproject_desc *desc, int32_t volumes);
int mvhmr_unproject_forward_shared(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords,
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_shared(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot, const float *center,
        const double position[3], const double sides[3],
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *coords,
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *rot,
        const float *center, const double position[3], const double sides[3],
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *coords,
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *rot, const float *center, const double position[3], const double sides[3],
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *coords,
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        float *grad_proj, float *grad_coords, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_shared(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *rot, const float *center, const double position[3], const double sides[3],
        int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
        float *grad_proj, float *grad_rot, float *grad_center, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Lens distortion (additive within ABI 4): the voxels are projected THROUGH a Brown-Conrady lens model, so the features may
 * come from raw, un-rectified images.  lens is (B,V,10) fp32 on the device, one record per (sample, view):
 *     fx, fy, cx, cy          the intrinsics that went into proj[b,v] (feature level; skew is taken as zero)
 *     k1, k2, p1, p2, k3      the distortion coefficients in OpenCV's order (the model of projectPoints, factors of two included)
 *     r2max                   the fold-back guard
 * With u = a / z, v = b / z the pin-hole pixel position of a voxel, every operation one separately rounded fp32 operation in this order:
 *     xn = (u - cx) / fx   yn = (v - cy) / fy   xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
 *     !(r2 <= r2max): the view gives this voxel an exactly zero sample, as z <= 0 does (nothing read, zero gradients; NaN compares false)
 *     rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *     xd = (xn*rad + (2*p1)*xy) + p2*(r2 + 2*xx)          yd = (yn*rad + p1*(r2 + 2*yy)) + (2*p2)*xy
 *     u' = fx*xd + cx      v' = fy*yd + cy
 * and u', v' take the place of u, v in everything that follows (grid normalisation, border tests, taps, weights).  A view whose five
 * coefficients are all +0.0 or -0.0 takes the plain path: its samples and gradients are bit-equal to the plain MVHMR_VARIANT_GATHER call
 * whatever its intrinsics say.  The gradients w.r.t. features, proj and coords / rot / center go through the lens (the geometry backward
 * multiplies by the 2x2 Jacobian of the step); the lens itself is not differentiated.
 * Routing: the gather kernels (MVHMR_VARIANT_AUTO runs them), planar or channels-last features, every storage mode of the plain gather
 * call; the feature backward takes the plane route wherever the plain MVHMR_VARIANT_GATHER call does.  MVHMR_VARIANT_BRICK and the
 * quad-planar layouts -> MVHMR_ERR_UNSUPPORTED ("lens distortion runs the gather kernels").  A null lens is the plain call with
 * MVHMR_VARIANT_GATHER.  view_mask, view_weights, view_confidence, visible and feature_index are the selections of the families above; they
 * do not compose with the lens yet: each must be null / 0, else MVHMR_ERR_UNSUPPORTED with its own text.
 * Workspace: no region is added; each *_lens_workspace_bytes total is the plain MVHMR_VARIANT_GATHER call's and covers the plain call's.
 */
size_t mvhmr_unproject_forward_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_forward_cuboid_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_deterministic_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_cuboid_deterministic_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
size_t mvhmr_unproject_backward_geometry_cuboid_lens_workspace_bytes(const mvhmr_unproject_desc *desc);
int mvhmr_unproject_forward_lens(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *coords,
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_forward_cuboid_lens(const mvhmr_unproject_desc *desc, const void *features, const float *proj, const float *rot, const float *center,
        const double position[3], const double sides[3],
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *out, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *coords,
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj, const float *rot,
        const float *center, const double position[3], const double sides[3],
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_deterministic_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *coords,
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_cuboid_deterministic_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *rot, const float *center, const double position[3], const double sides[3],
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        void *grad_features, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *coords,
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        float *grad_proj, float *grad_coords, void *workspace, size_t workspace_bytes, void *hip_stream);
int mvhmr_unproject_backward_geometry_cuboid_lens(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,
        const float *rot, const float *center, const double position[3], const double sides[3],
        const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,        float *grad_proj, float *grad_rot, float *grad_center, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The call record (additive within ABI 4): every un-projection call above as one struct, and the way in for new callers.
 * A named entry point fills a record from its arguments and calls the matching *_call function: the name's suffix is `family`, its
 * _cuboid infix is `placing`, its _deterministic infix is `deterministic`, its arguments are the fields.  Zero the record, set
 * struct_size = sizeof(mvhmr_unproject_call), then the fields the family takes:
 *
 *   family                    takes (beside features, proj, the placing and the outputs)    a null / zero field
 *   MVHMR_FAMILY_PLAIN        --
 *   MVHMR_FAMILY_MASKED       view_mask                                                      null mask: the plain call
 *   MVHMR_FAMILY_WEIGHTED     view_mask, view_weights; geometry: grad_weights                null weights: the masked (or plain) call
 *   MVHMR_FAMILY_VISIBLE      view_mask (the seeing test is always on)                       null mask: every view present
 *   MVHMR_FAMILY_CONFIDENCE   view_mask, view_confidence, visible; geometry: grad_confidence null maps: the visible / masked call, by `visible`
 *   MVHMR_FAMILY_SHARED       volumes, feature_index                                         null index: volumes == batch, the plain GATHER call
 *   MVHMR_FAMILY_LENS         lens                                                           null lens: the plain GATHER call
 *   MVHMR_FAMILY_MOMENTS      view_mask, visible, moments                                    moments 0: MVHMR_ERR_INVALID_ARGUMENT
 *
 * SHARED also carries view_mask, view_weights, view_confidence and visible, LENS those and feature_index: the selections that do not compose
 * with them yet, each refused with its own text (MVHMR_ERR_UNSUPPORTED).  Any other optional input a family does not take must be null / 0
 * (MVHMR_ERR_INVALID_ARGUMENT), and so must struct_size, family and placing be known values.  Everything else -- validation order, refusal
 * texts, kernels, bits, workspace sizes -- is that of the named call the record spells.
 * Placing: MVHMR_PLACING_TENSOR reads coords, MVHMR_PLACING_CUBOID rot, center and the HOST pointers position and sides (3 doubles each).
 * Per kind: forward reads features, proj and writes out; backward reads grad_out, features, proj and writes grad_features (bitwise
 * reproducible with `deterministic`); backward_geometry reads the same and writes grad_proj and grad_coords (tensor) or grad_rot, grad_center
 * (cuboid), grad_weights, grad_confidence -- each nullable, at least one given.
 * mvhmr_unproject_call_workspace_bytes answers from the descriptor and the record's family, placing, volumes and deterministic alone: it
 * reads no device pointer, so a record with only those fields set will do.
 */
typedef enum mvhmr_family_t {
    MVHMR_FAMILY_PLAIN = 0,
    MVHMR_FAMILY_MASKED = 1,
    MVHMR_FAMILY_WEIGHTED = 2,
    MVHMR_FAMILY_VISIBLE = 3,
    MVHMR_FAMILY_CONFIDENCE = 4,
    MVHMR_FAMILY_SHARED = 5,
    MVHMR_FAMILY_LENS = 6,
    MVHMR_FAMILY_MOMENTS = 7
} mvhmr_family_t;
typedef enum mvhmr_placing_t { MVHMR_PLACING_TENSOR = 0, MVHMR_PLACING_CUBOID = 1 } mvhmr_placing_t;
typedef enum mvhmr_call_kind_t { MVHMR_CALL_FORWARD = 0, MVHMR_CALL_BACKWARD = 1, MVHMR_CALL_GEOMETRY = 2 } mvhmr_call_kind_t;

typedef struct mvhmr_unproject_call {
    uint32_t struct_size;                       /* sizeof(mvhmr_unproject_call) */
    int32_t family;                             /* mvhmr_family_t */
    int32_t placing;                            /* mvhmr_placing_t */
    int32_t deterministic;                      /* backward only: non-zero = the deterministic form */
    int32_t volumes;                            /* SHARED: M */
    int32_t visible;                            /* CONFIDENCE, MOMENTS: non-zero = the seeing test */
    int32_t moments;                            /* MOMENTS: mvhmr_moments_t */
    int32_t reserved;                           /* 0 */
    const float *coords;                        /* tensor placing */
    const float *rot, *center;                  /* cuboid placing */
    const double *position, *sides;             /*   (host, 3 doubles each) */
    const uint8_t *view_mask;
    const float *view_weights, *view_confidence;
    const int32_t *feature_index;
    const float *lens;
    const void *features;
    const float *proj;
    const void *grad_out;
    void *out, *grad_features;
    float *grad_proj, *grad_coords, *grad_rot, *grad_center, *grad_weights, *grad_confidence;
} mvhmr_unproject_call;

size_t mvhmr_unproject_call_workspace_bytes(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, int kind /* mvhmr_call_kind_t */);
int mvhmr_unproject_forward_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace, size_t workspace_bytes,
                                 void *hip_stream);
int mvhmr_unproject_backward_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace, size_t workspace_bytes,
                                  void *hip_stream);
int mvhmr_unproject_backward_geometry_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace,
                                           size_t workspace_bytes, void *hip_stream);

/*
 * Layout pass on its own: features (B,V,C,Hf,Wf) -> dst in `dst_layout` (MVHMR_LAYOUT_BVHWC with the channel
 * count rounded up to a multiple of 4 and zero padded, or MVHMR_LAYOUT_QUAD), desc->feat_dtype.
 * desc->feat_layout names the SOURCE: MVHMR_LAYOUT_BVCHW (also assumed for MVHMR_LAYOUT_QUAD descriptors, as before), or
 * MVHMR_LAYOUT_BVHWC -- channels-last features to MVHMR_LAYOUT_QUAD only (how a channels-last caller reaches the brick kernels).
 * mvhmr_unproject_forward runs the pass its kernel needs into its workspace when desc->feat_layout is
 * MVHMR_LAYOUT_BVCHW; callers that keep the converted copy (or time the two kernels separately) call this and
 * then pass desc->feat_layout = dst_layout.  mvhmr_preferred_layout says which layout the kernel that
 * desc->variant selects reads; dst needs mvhmr_feature_layout_bytes(desc, dst_layout) bytes.
 */
int mvhmr_preferred_layout(const mvhmr_unproject_desc *desc);
size_t mvhmr_feature_layout_bytes(const mvhmr_unproject_desc *desc, int dst_layout);
int mvhmr_convert_features(const mvhmr_unproject_desc *desc, const void *features, int dst_layout, void *dst,
                           void *hip_stream);

/*
 * process_feature (the 1x1 conv in front of the un-projection, models/aggregation.py:108-110,189-191) fused with the layout pass:
 *     y[m, co, p] = sum_ci weight[co, ci] * x[m, ci, p] + bias[co]          m = (b, v),  p = (y, x)
 * computed as an fp32 MFMA GEMM whose epilogue writes dst in MVHMR_LAYOUT_QUAD (n_maps, c_out/4, Wf, Hf, 4) -- feed it to
 * mvhmr_unproject_forward[_cuboid] with desc->feat_layout = MVHMR_LAYOUT_QUAD and the planar conv output and the layout pass
 * never exist (variant AUTO: the brick kernels read the copy as it is; when the geometry gate picks the gather kernels they get a
 * channels-last conversion of it).  mvhmr_unproject_backward[_cuboid] accepts the same MVHMR_LAYOUT_QUAD features and
 * then writes grad_features in the PLANAR layout (n_maps, c_out, Hf, Wf), which is what the conv's own backward consumes.
 *   x (n_maps, c_in, Hf, Wf) fp32, weight (c_out, c_in) fp32 (nn.Conv2d's (c_out, c_in, 1, 1)), bias (c_out) fp32 or null.
 * Shapes: c_in % 16 == 0, c_out % 128 == 0, Hf % 4 == 0, Wf % 32 == 0 (mvhmr_conv1x1_to_quad_supported), else MVHMR_ERR_UNSUPPORTED.
 * n_maps <= 65535 (the maps are the grid's z extent), else MVHMR_ERR_UNSUPPORTED: split the batch.  Element offsets are 64-bit: a tensor
 * may hold more than 2^31 elements.
 * Alignment (this and the three GEMMs below): the kernels use 16-byte loads and stores, so x, weight, bias (when given) and dst here and
 * in mvhmr_conv1x1_planar, grad_y and x in mvhmr_conv1x1_wgrad[_deterministic], must be 16-byte aligned, else
 * MVHMR_ERR_INVALID_ARGUMENT (every map and weight row then is, by the shape rules).  Checks run in this order: null pointers,
 * non-positive extents, alignment (MVHMR_ERR_INVALID_ARGUMENT), then shape and n_maps (MVHMR_ERR_UNSUPPORTED), then the workspace.
 */
int mvhmr_conv1x1_to_quad(const float *x, const float *weight, const float *bias, void *dst, int32_t n_maps, int32_t c_in,
                          int32_t c_out, int32_t feat_h, int32_t feat_w, void *hip_stream);
int mvhmr_conv1x1_to_quad_supported(int32_t c_in, int32_t c_out, int32_t feat_h, int32_t feat_w);

/*
 * The same fp32 MFMA GEMM with a planar result: dst (n_maps, c_out, pixels) = weight (c_out, c_in) @ x (n_maps, c_in, pixels)
 * (+ bias).  With the transposed weight it is the gradient w.r.t. the input of process_feature (autograd through
 * models/aggregation.py:189-191), which the Python binding's fused route uses in backward.
 * Shapes: c_in % 16 == 0, c_out % 128 == 0, pixels % 128 == 0 (mvhmr_conv1x1_planar_supported), else MVHMR_ERR_UNSUPPORTED.
 * n_maps <= 65535 and 16-byte aligned x, weight, bias, dst as for mvhmr_conv1x1_to_quad.
 */
int mvhmr_conv1x1_planar(const float *x, const float *weight, const float *bias, float *dst, int32_t n_maps, int32_t c_in,
                         int32_t c_out, int32_t pixels, void *hip_stream);
int mvhmr_conv1x1_planar_supported(int32_t c_in, int32_t c_out, int32_t pixels);

/*
 * Weight and bias gradient of process_feature (autograd through models/aggregation.py:189-191):
 *     grad_weight[co, ci] += sum over maps and pixels of grad_y[n, co, p] * x[n, ci, p]      grad_bias[co] += sum of grad_y[n, co, p]
 * grad_y (n_maps, c_out, pixels), x (n_maps, c_in, pixels) fp32 planar.  grad_weight (c_out, c_in) and grad_bias (c_out, may be
 * NULL) are ADDED INTO with float atomics (zero them first; last-bit run-to-run differences like any split-K reduction).
 * Shapes: c_in % 128 == 0, c_out % 128 == 0, pixels % 32 == 0 (mvhmr_conv1x1_wgrad_supported), else MVHMR_ERR_UNSUPPORTED.
 * grad_y and x must be 16-byte aligned (MVHMR_ERR_INVALID_ARGUMENT); n_maps has no limit of its own here.
 */
int mvhmr_conv1x1_wgrad(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int32_t n_maps, int32_t c_in,
                        int32_t c_out, int32_t pixels, void *hip_stream);
int mvhmr_conv1x1_wgrad_supported(int32_t c_in, int32_t c_out, int32_t pixels);

/*
 * Deterministic mvhmr_conv1x1_wgrad: the same arguments, shapes and error codes, but grad_weight and grad_bias are WRITTEN (not added
 * into) and bitwise reproducible: every block stores its partial tile into a slab of `workspace`, a second kernel sums the slabs per
 * element in a fixed order (float64).  Workspace: mvhmr_conv1x1_wgrad_deterministic_workspace_bytes, 256-byte aligned: one partial
 * (c_out x c_in + c_out) fp32 slab per pixel slice, n_maps * slices_per_map slices.  Each map is split into as many slices as keep the grid
 * at most 2048 blocks of 128 x 128 (about 128 MB); with n_maps * (c_out / 128) * (c_in / 128) > 2048 every map is one slice and the size is
 * n_maps * (c_out * c_in + c_out) * 4 bytes.
 */
size_t mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(int32_t n_maps, int32_t c_in, int32_t c_out, int32_t pixels);
int mvhmr_conv1x1_wgrad_deterministic(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int32_t n_maps,
                                      int32_t c_in, int32_t c_out, int32_t pixels, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * DLT triangulation of one 3-D point per sample from its V views: replaces triangulate_point_from_multiple_views_linear[_torch]
 * (utils/multiview.py:112-168) where VolumeGenerator.forward calls it per sample with a device SVD and a .cpu() each
 * (models/aggregation.py:174-177).  Homogeneous solution of A h = 0 (rows u P[2,:] - P[0,:], v P[2,:] - P[1,:]) as the smallest
 * eigenvector of the normal matrix A^T A (the unit-norm least-squares solution, as the SVD gives it), float64 Jacobi rotations, one
 * thread per sample, no host synchronisation.
 *   proj    (B,V,3,4) fp32, device      points  (V,2) fp32 shared by the samples (points_per_sample = 0) or (B,V,2) (= 1), device
 *   out     (B,3) fp32, device
 */
int mvhmr_triangulate_dlt(const float *proj, const float *points, float *out, int32_t batch, int32_t views,
                          int32_t points_per_sample, void *hip_stream);
/* the same with the per-view confidences of triangulate_point_from_multiple_views_linear_torch (utils/multiview.py:156-161: both rows of
 * view v are multiplied by c_v before the decomposition): confidences (V) fp32 shared by the samples (confidences_per_sample = 0) or (B,V) */
int mvhmr_triangulate_dlt_weighted(const float *proj, const float *points, const float *confidences, float *out, int32_t batch, int32_t views,
                                   int32_t points_per_sample, int32_t confidences_per_sample, void *hip_stream);
/*
 * Backward of the DLT: the gradient torch.svd's backward gives through the reference's -vh[:, 3] (sign-invariant), from the eigenpairs
 * of the same normal matrix, float64, one thread per sample.
 *   confidences  (V) / (B,V) fp32 as for mvhmr_triangulate_dlt_weighted, or NULL (every weight 1)
 *   grad_out     (B,3) fp32                                                                          [read]
 *   grad_proj    (B,V,3,4) fp32 or NULL; grad_points (B,V,2) fp32 or NULL; grad_conf (B,V) fp32 or NULL   [write]
 * grad_points and grad_conf are always per sample, also when points / confidences are shared: the caller sums them over the batch.
 * At least one output must be non-null.  views >= 1: a sample with fewer than 2 views, or whose normal matrix has a repeated smallest
 * eigenvalue (|l_k - l_min| <= 1e-12 l_max for some other eigenvalue l_k), has no gradient -- every output of that sample is NaN (the
 * reference's SVD backward is non-finite there, or fails outright at V = 1).
 */
int mvhmr_triangulate_dlt_backward(const float *proj, const float *points, const float *confidences, const float *grad_out, float *grad_proj,
                                   float *grad_points, float *grad_conf, int32_t batch, int32_t views, int32_t points_per_sample,
                                   int32_t confidences_per_sample, void *hip_stream);

/*
 * Caller-side helper of VolumeGenerator.forward (models/aggregation.py:138-187): fills
 * coords (B,S,S,S,3) fp32 with the cuboid grid `position + side/(S-1) * (i,j,k)` rotated by
 * rot[b] (3x3 row-major fp32, utils/volumetric.py:87-114) about center[b] (3 fp32):
 *     coords = rot @ (grid - center) + center
 * position is the cuboid corner, sides its edge lengths (3 doubles each, HOST memory, as the reference
 * holds them in float64 numpy, aggregation.py:143-144); rot / center / coords are device pointers.
 */
int mvhmr_build_coord_volumes(float *coords, const float *rot, const float *center, int32_t batch,
                              int32_t volume_size, const double position[3], const double sides[3],
                              void *hip_stream);

/*
 * Volumetric 3-D soft-argmax (additive within ABI 4): keypoints from (B,J,X,Y,Z) heat volumes without a softmaxed
 * copy and -- on the cuboid route -- without coordinate volumes.  Per slice (b,j), N = X*Y*Z, flat index n = (i*Y + j')*Z + k:
 *     p_n = exp(beta v_n) / sum_m exp(beta v_m)      L = ln sum_m exp(beta v_m)      mu = sum_n p_n u_n          (fp32 arithmetic)
 * Tensor route (coords non-null): u_n = coords[b,n,:], keypoint = mu.  Cuboid route (coords NULL): u_n is the un-rotated offset
 * (position + step*index) - center[b] in the roundings of mvhmr_build_coord_volumes, keypoint = rot[b] mu + center[b] in its FMA order.
 *   volumes      (B,J,X,Y,Z) of `dtype` (MVHMR_F32 / MVHMR_F16 / MVHMR_BF16), device                              [read]
 *   coords       (B,X,Y,Z,3) fp32, device, or NULL: then rot (B,9), center (B,3) fp32 device, position / sides 3 host doubles each
 *   beta         finite; it is rounded to fp32 (as beta * log2(e)) before it meets the volume
 *   keypoints    (B,J,3) fp32     logsumexp (B,J) fp32     moment (B,J,3) fp32: mu in the accumulation frame    [write, all non-null]
 *   workspace    mvhmr_soft_argmax3d_workspace_bytes(...) bytes, 16-byte aligned: the per-split records
 * A -inf entry beside finite ones contributes exactly 0; a slice holding a NaN, +inf or nothing but -inf gives NaN in all three outputs.
 * Sizes: every extent >= 1, N < 2^31, B*J <= 2^31 - 1 (MVHMR_ERR_INVALID_ARGUMENT otherwise); unknown dtype: MVHMR_ERR_INVALID_ARGUMENT; a null,
 * short or misaligned workspace: MVHMR_ERR_WORKSPACE.  No atomics: every output is bitwise reproducible.  The number of blocks a slice is
 * split over, mvhmr_soft_argmax3d_splits, is a function of the sizes alone (never of the device), so results do not depend on the card.
 */
int32_t mvhmr_soft_argmax3d_splits(int32_t batch, int32_t joints, int64_t voxels);
size_t mvhmr_soft_argmax3d_workspace_bytes(int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z);
int mvhmr_soft_argmax3d_forward(const void *volumes, int32_t dtype, const float *coords, const float *rot, const float *center,
                                const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                int32_t vol_z, double beta, float *keypoints, float *logsumexp, float *moment, void *workspace,
                                size_t workspace_bytes, void *hip_stream);
/*
 * Its backward w.r.t. the volume: with g = grad_keypoints (B,J,3), g_L = grad_logsumexp (B,J) (each fp32 or NULL = zero; both NULL is
 * MVHMR_ERR_INVALID_ARGUMENT), h = g on the tensor route and rot[b]^T g on the cuboid route,
 *     grad_volumes[n] = beta p_n (h . (u_n - mu) + g_L),     p_n = exp(beta v_n - L) recomputed from logsumexp, never stored
 * logsumexp and moment are the forward's outputs; grad_volumes (B,J,X,Y,Z) is written in `dtype`.  No workspace.
 */
int mvhmr_soft_argmax3d_backward(const void *volumes, int32_t dtype, const float *coords, const float *rot, const float *center,
                                 const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                 int32_t vol_z, double beta, const float *logsumexp, const float *moment, const float *grad_keypoints,
                                 const float *grad_logsumexp, void *grad_volumes, void *hip_stream);
/* tensor route: grad_coords[b,n,:] = sum_j p_{j,n} g_{b,j,:}, j in index order; (B,X,Y,Z,3) fp32 */
int mvhmr_soft_argmax3d_backward_coords(const void *volumes, int32_t dtype, int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                        int32_t vol_z, double beta, const float *logsumexp, const float *grad_keypoints, float *grad_coords,
                                        void *hip_stream);
/* cuboid route: grad_rot[b] = sum_j g_{b,j} mu_{b,j}^T (B,9), grad_center[b] = sum_j (g_{b,j} - rot[b]^T g_{b,j}) (B,3), j in index order;
 * either output may be NULL, not both */
int mvhmr_soft_argmax3d_backward_pose(const float *rot, const float *moment, const float *grad_keypoints, float *grad_rot, float *grad_center,
                                      int32_t batch, int32_t joints, void *hip_stream);

/*
 * Trilinear volume sampling at world points (additive within ABI 4): reads (B,C,X,Y,Z) volumes that live on the cuboid
 * recipe of mvhmr_build_coord_volumes -- voxel (i,j,k) at rot (position + step*(i,j,k) - center) + center, step_a = fl32(sides_a / (S_a - 1))
 * -- back at N world points per sample.  The inverse uses rot^T: rot must be orthonormal (not checked).  Per point x, every line one
 * rounded fp32 operation, volume values widened to fp32 first:
 *     y_i = x_i - c_i      d_a = fma(R[2][a], y_2, fma(R[1][a], y_1, R[0][a] * y_0))      o_a = c_a - fl32(position_a)
 *     t_a = (d_a + o_a) / step_a                                                       -> index, the continuous voxel index
 *     unless -1 < t_a < S_a on every axis (a NaN fails): sample 0 and no gradient through this point
 *     i0 = floor(t), w1 = t - i0, w0 = (i0 + 1) - t, w(dx,dy,dz) = (wx * wy) * wz; a tap outside the grid counts as value 0
 *     sample = fma chain over the taps in the order dx*4 + dy*2 + dz; a tap whose weight is exactly 0 is not read
 * (zero padding, align_corners = True; the last rule is the one departure from a 5-D grid_sample: a point on a lattice node returns the
 * node's value whatever its neighbours hold, -inf included).
 *   volumes      (B,C,X,Y,Z) of `dtype` (MVHMR_F32 / MVHMR_F16 / MVHMR_BF16), device                                [read]
 *   points       (B,N,3) fp32 world coordinates; rot (B,9), center (B,3) fp32, device; position / sides 3 host doubles each
 *   paired       0: every point samples every channel, samples is (B,C,N).  1: requires N == C, point j samples channel j, samples is (B,C)
 *   samples      fp32 [write]       index (B,N,3) fp32 [write]; reported for points outside the volume too, NaN for a NaN point
 * Sizes: batch, channels, points >= 1, every extent >= 2, X*Y*Z < 2^31, B*C and B*N below 2^31 (MVHMR_ERR_INVALID_ARGUMENT otherwise, as for
 * an unknown dtype or a null pointer).  No atomics anywhere: every output and gradient is bitwise reproducible.
 */
int32_t mvhmr_sample_volume_chunk_points(void);
size_t mvhmr_sample_volume_workspace_bytes(int32_t batch, int32_t points);
int mvhmr_sample_volume_forward(const void *volumes, int32_t dtype, const float *points, const float *rot, const float *center,
                                const double position[3], const double sides[3], int32_t batch, int32_t channels, int32_t vol_x, int32_t vol_y,
                                int32_t vol_z, int32_t n_points, int32_t paired, float *samples, float *index, void *hip_stream);
/*
 * Its backward w.r.t. the volume, from the forward's index and g = grad_samples (shaped like samples): grad_volumes (B,C,X,Y,Z) in `dtype`
 * is zero-filled by the call, then grad_volumes[b,c,voxel] = sum of w * g[b,c,n] over the taps of nonzero weight that land on the voxel, in
 * ascending point index by acc = fma(w, g, acc), the first term w * g.  Points are taken in chunks of mvhmr_sample_volume_chunk_points()
 * (a constant of the library): per chunk the taps are sorted by (voxel, point) into the workspace, every voxel gets one owner, and the owner
 * adds its chunk's sum to the stored value -- a 16-bit grad_volumes is therefore rounded once per chunk that touches the voxel.
 *   workspace    mvhmr_sample_volume_workspace_bytes(batch, points) bytes, 16-byte aligned (a function of the two sizes alone); a null,
 *                short or misaligned one is MVHMR_ERR_WORKSPACE (a paired call has no collisions and leaves it untouched, the rule holds all the same).
 */
int mvhmr_sample_volume_backward_volumes(int32_t dtype, const float *index, const float *grad_samples, int32_t batch, int32_t channels,
                                         int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t n_points, int32_t paired, void *grad_volumes,
                                         void *workspace, size_t workspace_bytes, void *hip_stream);
/*
 * Its backward w.r.t. the geometry.  With q = dL/dt (out-of-grid taps count as value 0, the cell is floor(t); channels summed in index
 * order) and u = q / step:
 *     grad_points[b,n] = rot_b u_n      grad_rot[b][i][a] = sum_n y_{n,i} u_{n,a}      grad_center[b] = sum_n (u_n - rot_b u_n)
 * the sums over n in index order.  grad_points (B,N,3), grad_rot (B,9), grad_center (B,3) fp32 may each be NULL, not all of them.  The
 * workspace (same query, same rules) holds u.
 */
int mvhmr_sample_volume_backward_geometry(const void *volumes, int32_t dtype, const float *points, const float *rot, const float *center,
                                          const double position[3], const double sides[3], int32_t batch, int32_t channels, int32_t vol_x,
                                          int32_t vol_y, int32_t vol_z, int32_t n_points, int32_t paired, const float *index,
                                          const float *grad_samples, float *grad_points, float *grad_rot, float *grad_center, void *workspace,
                                          size_t workspace_bytes, void *hip_stream);

/*
 * 3-D non-maximum suppression and top-K proposals from heat volumes (additive within ABI 4).  Per slice (b, j) of volumes
 * (B,J,X,Y,Z), voxel n = (i*Y + j)*Z + k is a PEAK iff, with the box [i-r, i+r] x [j-r, j+r] x [k-r, k+r] clipped to the volume,
 *     no value in the box is NaN (the centre included),      v_n >= every value in the box (equal neighbours do not suppress each other:
 *     a plateau is all peaks; -0 and +0 are equal),          v_n > threshold, strictly (values widened to fp32, threshold an fp32).
 * threshold = -inf keeps every peak but a -inf voxel, which is never one; +inf can be one.  radius r is 0 .. 3 (0: no suppression) and may
 * exceed an extent.  The K outputs of a slice are its peaks by value descending, ties by ascending n; slots beyond the number of peaks
 * hold scores = -inf, index = -1, positions = 0.  Every output is a function of the input bits alone (no float atomics; the integer
 * counters inside a block only order work that is sorted afterwards by distinct keys).
 *   volumes      (B,J,X,Y,Z) of `dtype` (MVHMR_F32 / MVHMR_F16 / MVHMR_BF16), device                                  [read]
 *   scores       (B,J,K) fp32: the stored values, widened [write]         index (B,J,K) int32 [write]
 *   positions    (B,J,K,3) fp32 or NULL.  Non-null needs rot (B,9), center (B,3) fp32 on the device and position / sides, 3 host doubles
 *                each: the voxel's world coordinate by the cuboid recipe, bit-equal to mvhmr_build_coord_volumes' entry at that index.
 *                With positions NULL the four cuboid pointers are not read and may be NULL                              [write]
 *   workspace    mvhmr_volume_peaks_workspace_bytes(...) bytes, 16-byte aligned: blocks_per_slice * K 64-bit keys per slice, whatever the
 *                volume holds (a constant volume, where every voxel is a peak, included)
 * Checked in this order, before anything is launched: null pointers, batch / joints / extents >= 1, X*Y*Z and B*J below 2^31, 1 <= k <=
 * mvhmr_volume_peaks_max_k(), 0 <= radius <= 3, a NaN threshold (MVHMR_ERR_INVALID_ARGUMENT); an unknown dtype, or more blocks than one
 * launch holds (MVHMR_ERR_UNSUPPORTED); the workspace (MVHMR_ERR_WORKSPACE).
 * mvhmr_volume_peaks_tile: the extents (X run, Y tile, Z tile) of the strip of a slice that one block owns; blocks_per_slice is the
 * product of ceil(extent / tile) over the three axes.  Constants of the library, for tests that want shapes on both sides of a tile edge.
 */
void mvhmr_volume_peaks_tile(int32_t tile[3]);
int32_t mvhmr_volume_peaks_max_k(void);
size_t mvhmr_volume_peaks_workspace_bytes(int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t k);
int mvhmr_volume_peaks(const void *volumes, int32_t dtype, int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t k,
                       int32_t radius, float threshold, const float *rot, const float *center, const double position[3], const double sides[3],
                       float *scores, int32_t *index, float *positions, void *workspace, size_t workspace_bytes, void *hip_stream);
/*
 * Its backward w.r.t. the volume: grad_volumes (B,J,X,Y,Z) in `dtype` is zero-filled by the call, then grad_volumes[b,j,index[b,j,s]] =
 * grad_scores[b,j,s] (rounded once to `dtype`) for every slot with index >= 0.  The indices of a slice are distinct: plain stores.
 */
int mvhmr_volume_peaks_backward(int32_t dtype, const int32_t *index, const float *grad_scores, int32_t batch, int32_t joints, int32_t vol_x,
                                int32_t vol_y, int32_t vol_z, int32_t k, void *grad_volumes, void *hip_stream);
/*
 * The backward of positions w.r.t. the pose.  x = rot d + center with d = grid - center (the recipe's un-rotated offset, recomputed from
 * index), g = grad_positions (B,J,K,3):  grad_rot[b][r][c] = sum g_r d_c by acc = fma(g_r, d_c, acc),  grad_center[b][c] = sum (g_c -
 * (rot^T g)_c) by acc = acc + (g_c - h_c), both over the slots of sample b with index >= 0 in (j, slot) order.  grad_rot (B,9) and
 * grad_center (B,3) fp32 may each be NULL, not both.  Nothing is differentiated through index.
 */
int mvhmr_volume_peaks_backward_pose(const int32_t *index, const float *grad_positions, const float *rot, const float *center,
                                     const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                     int32_t vol_z, int32_t k, float *grad_rot, float *grad_center, void *hip_stream);

/*
 * Ray-marching volumes into camera-view maps (additive within ABI 4): renders (B,C,X,Y,Z) volumes that live on the cuboid
 * recipe into maps (B,V,C,Hm,Wm), the direction opposite to un-projection.  rays (B,V,3,4) fp32 holds [D | o] per view: with the
 * projection P = [M | p4], D = M^-1 and o = -M^-1 p4, so the world point of pixel (u, v) = (column, row) at parameter lambda is
 * o + lambda D (u, v, 1)^T and projects back to (u, v) with homogeneous w = lambda.  Per ray, every line one rounded fp32 operation:
 *     t_o = the index of o as mvhmr_sample_volume_forward computes it      d_i = fma(D[i][1], v, fma(D[i][0], u, D[i][2]))
 *     r_a = fma(R[2][a], d_2, fma(R[1][a], d_1, R[0][a] * d_0))            e_a = r_a / step_a
 *     slab clip against 0 <= t_a <= S_a - 1, axes in order: e_a == 0 misses unless t_o,a lies in the slab; else l0 = (0 - t_o,a) / e_a,
 *     l1 = ((S_a - 1) - t_o,a) / e_a, lin = max(min_depth, the smaller of each pair), lout = min(max_depth, the larger); a NaN is a miss
 *     hit iff lin < lout, both finite      h = (lout - lin) / K      lam_k = fma(k + 0.5, h, lin)      t_k,a = fma(lam_k, e_a, t_o,a)
 *     s_k = the sample at index t_k by mvhmr_sample_volume_forward's tap rule
 * method (mvhmr_project_t), over k ascending: MEAN  acc = acc + s_k, out = acc / K.   MAX  the maximum, the lowest k that attains it.
 * SOFTMAX  sum_k p_k s_k, p = softmax_k(beta s_k), by the running-maximum recurrence at the top of volume_project.hip; beta finite, != 0.
 * A miss gives 0 in every channel, ranges (0, 0), and takes part in no gradient.
 *   volumes      (B,C,X,Y,Z) of `dtype` (MVHMR_F32 / MVHMR_F16 / MVHMR_BF16), device                                [read]
 *   rays         (B,V,3,4) fp32; rot (B,9), center (B,3) fp32, device; position / sides 3 host doubles each
 *   maps         (B,V,C,Hm,Wm) fp32 [write]       ranges (B,V,Hm,Wm,2) fp32: (lin, lout) per ray [write]
 *   aux          (B,V,C,Hm,Wm) 4-byte words the backward reads: MAX the arg-k (int32), SOFTMAX the log-sum-exp of beta s_k (fp32); MEAN: may be NULL
 * Sizes: batch, views, channels, map extents >= 1, every volume extent >= 2, 1 <= n_samples <= mvhmr_project_volume_max_samples(),
 * X*Y*Z, B*C*V and V*Hm*Wm*n_samples below 2^31; min_depth finite, max_depth not NaN (MVHMR_ERR_INVALID_ARGUMENT otherwise).
 */
typedef enum {
    MVHMR_PROJECT_MEAN = 0,
    MVHMR_PROJECT_MAX = 1,
    MVHMR_PROJECT_SOFTMAX = 2
} mvhmr_project_t;
int32_t mvhmr_project_volume_max_samples(void);
/* (channels per block, channels per trip of a sample's channel loop): constants of the library, for tests that want channel counts on
 * both sides of either boundary */
void mvhmr_project_volume_channel_group(int32_t group_unroll[2]);
size_t mvhmr_project_volume_workspace_bytes(int32_t batch, int32_t channels, int32_t vol_x, int32_t vol_y, int32_t vol_z);
int mvhmr_project_volume_forward(const void *volumes, int32_t dtype, const float *rays, const float *rot, const float *center,
                                 const double position[3], const double sides[3], int32_t batch, int32_t views, int32_t channels, int32_t vol_x,
                                 int32_t vol_y, int32_t vol_z, int32_t map_h, int32_t map_w, int32_t n_samples, int32_t method, double beta,
                                 double min_depth, double max_depth, float *maps, float *ranges, void *aux, void *hip_stream);
/*
 * Its backward w.r.t. the volume, from g = grad_maps (B,V,C,Hm,Wm) fp32 and the forward's maps and aux: the rays are marched again and every
 * live tap adds w * ds_k -- ds_k = g / K (MEAN), g at the saved k (MAX), (g p_k) * fma(beta, s_k - out, 1) with p_k = exp(beta s_k - lse)
 * (SOFTMAX) -- to an int64 fixed-point accumulator with 64-bit integer atomics; one exponent per (b, c), chosen before any add so that no
 * sum can overflow.  Integer adds are associative: grad_volumes (B,C,X,Y,Z) in `dtype`, fully written by the call, is bitwise
 * reproducible.  A (b, c) whose grad_maps rows (or, SOFTMAX, whose volume) hold a non-finite value comes back NaN.
 *   workspace    mvhmr_project_volume_workspace_bytes(...) bytes, 16-byte aligned: three B*C tables and the accumulator of one pass of
 *                channels, 8 bytes per voxel and channel, as many channels as keep it within 2^30 bytes (one at the least); a null,
 *                short or misaligned one is MVHMR_ERR_WORKSPACE
 */
int mvhmr_project_volume_backward_volumes(const void *volumes, int32_t dtype, const float *rays, const float *rot, const float *center,
                                          const double position[3], const double sides[3], int32_t batch, int32_t views, int32_t channels,
                                          int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t map_h, int32_t map_w, int32_t n_samples,
                                          int32_t method, double beta, double min_depth, double max_depth, const float *grad_maps,
                                          const float *maps, const void *aux, void *grad_volumes, void *workspace, size_t workspace_bytes,
                                          void *hip_stream);

/* Which kernel AUTO would run for this problem (an mvhmr_variant_t), for logs and tests. */
int mvhmr_unproject_selected_variant(const mvhmr_unproject_desc *desc);

/*
 * Planning query for callers that run the layout pass themselves (mvhmr_convert_features + an explicit layout, which the
 * device-side gate does not cover): the variant (mvhmr_variant_t) the gate would select for THIS geometry, or -1 on error.
 * SYNCHRONOUS -- allocates 4 bytes, runs the gate kernel on hip_stream and waits for it: for set-up code, never for the
 * per-step path.  proj (B,V,3,4) and coords (B,X,Y,Z,3) as for mvhmr_unproject_forward.
 */
int mvhmr_unproject_query_variant(const mvhmr_unproject_desc *desc, const float *proj, const float *coords,
                                  void *hip_stream);
int mvhmr_unproject_query_variant_cuboid(const mvhmr_unproject_desc *desc, const float *proj, const float *rot,
                                         const float *center, const double position[3], const double sides[3],
                                         void *hip_stream);

/* Testing hook: the key under which the library remembers that it raised a kernel's dynamic-LDS limit (the attribute is
 * per device AND kernel; a second GPU driven from the same process must get its own opt-in). */
unsigned long long mvhmr_internal_lds_cache_key(int device, const void *kernel);

/* Testing hook: where a deterministic feature backward keeps its exponent table K[b][c] (int32, batch * channels entries; the scale pass
 * of DESIGN.md 5.7 writes it before any tap is added).  Answered from the plan alone -- the descriptor and what the record selects; no
 * device pointer is read: *offset is the table's byte offset inside the caller's workspace, *count its length.  `call` is a backward
 * record with `deterministic` set, checked and refused as mvhmr_unproject_backward_call would; a plan that takes the plane route has no
 * scale pass and answers MVHMR_ERR_UNSUPPORTED ("... no scale pass"). */
int mvhmr_internal_det_exponent_table(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, size_t *offset, size_t *count);

int mvhmr_abi_version(void);
const char *mvhmr_status_string(int status);
const char *mvhmr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MVHMR_UNPROJECT_H */
