// Host-visible launchers of the HIP kernels (internal to the library; the public ABI is include/mvhmr_unproject.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "gate.h"

namespace mvhmr {

struct Problem {
    int B, V, C, H, W;        // features (B,V,C,H,W)
    int X, Y, Z;              // volume
    long long N;              // X*Y*Z
    int C4;                   // channels rounded up to a multiple of 4 (channels-last row length)
    int method;               // AGG_*
    int feat_f16, out_f16;    // storage types
    int out_bf16 = 0;         // the volume (out / grad_out) is bf16; features are fp32 then
    int feat_log2e = 0;       // forward, quad-planar copy: the staged features are multiplied by log2(e) (brick_fwd_prescales)
    // Geometry gate (AUTO on planar input, shapes both variants serve): `gate_count` points at a device counter of
    // bricks whose windows overflow LDS (k_brick_gate); a gated kernel runs when (count <= gate_limit) == wants_brick
    // and returns at once otherwise.  Null = no gate.
    const int *gate_count = nullptr;
    int gate_limit = 0;
    // View masks: per-sample count of present views (device, B ints), which the layout pass packed into view slots
    // 0 .. n_b - 1 of every sample.  Null = every view present; the kernels that take it (gather, geometry) launch MASK instances.
    const int *view_count = nullptr;
    // Per-view confidence weights: the packed weights (device, (B, V) fp32 in slot order, > 0 for the view_count[b] present
    // views, 0 behind them).  Null = unweighted; set together with view_count, the kernels that take it launch their weighted instances.
    const float *view_weights = nullptr;
    // the view-mask route (set before the table exists, for the workspace queries): the gather family with the per-tap scatter backward
    int masked = 0;
    // Visibility-aware aggregation: every voxel aggregates only the views that see it.  The gather and geometry launchers
    // hand such a problem to their *_seen kernels (unproject_visible.hip, unproject_visible_geom.hip); view_count, when set, bounds the slots.
    int visible = 0;
    // Per-pixel view confidence: the maps (device, (B, V, Hf, Wf) fp32, in slot order when view_count is set), sampled like one
    // more channel; a view takes part for a voxel iff its sample is > 0 (and, with `visible`, it sees the voxel).  Null = none; the gather and
    // geometry launchers hand such a problem to their *_conf kernels (unproject_confidence.hip, unproject_confidence_geom.hip).  `conf` marks
    // the route before the pointer exists (the workspace queries); conf_stream, when set, receives the geometry kernel's (B, V, N) fp32 stream
    // of sum_channels dc (conf_grad_stream_bytes), from which launch_conf_grad builds grad_confidence.
    const float *confidence = nullptr;
    int conf = 0;
    float *conf_stream = nullptr;
    // Shared feature maps: `volumes` (M) volumes read the B feature samples through feature_index (device, M ints): volume m
    // un-projects features[feature_index[m]] under proj[feature_index[m]] onto coordinates / pose / output m; an entry outside [0, B) is "no
    // sample" (a zero volume that contributes to no gradient).  Null = volume b reads sample b (volumes is not read).  The host route hands
    // such a problem to the *_shared kernels (unproject_shared.hip, unproject_shared_geom.hip); B stays the number of FEATURE samples.
    const int *feature_index = nullptr;
    int volumes = 0;
    // Lens distortion: one Brown-Conrady record per (sample, view) (device, (B, V, 10) fp32: fx, fy, cx, cy, k1, k2, p1, p2,
    // k3, r2max; lens.h) through which the voxels are projected.  Null = pin-hole cameras.  The host route hands such a problem to the *_lens
    // kernels (unproject_lens.hip, unproject_lens_geom.hip); the plane backward builds its tap table through the records and runs as it is.
    const float *lens = nullptr;
    // Cross-view variance: 1 = the volume holds the population variance of the participating views' samples (C channels),
    // 2 = their mean and that variance (2C channels: mean first).  0 = the first-order aggregate of `method`.  The participating set is every
    // present view, or -- with `visible` -- the present views that see the voxel.  The host route hands such a problem to the *_moments kernels
    // (unproject_moments.hip, unproject_moments_geom.hip): the gather family with the per-tap scatter backward.
    int moments = 0;
};

inline Gate make_gate(const Problem &p, bool wants_brick) { return Gate{p.gate_count, p.gate_limit, wants_brick ? 1 : 0}; }


// Raises a kernel's dynamic-LDS limit once per (device, kernel), remembering the largest size asked for: the attribute call
// is not a stream operation, so it is kept off the per-launch path and out of graph captures after the first (warm-up)
// launch.  hipFuncSetAttribute acts on the CURRENT device's function object, hence the device in the key.
hipError_t allow_dynamic_lds(const void *kernel, size_t bytes);
// the cache key (exposed for the unit test of the key)
unsigned long long dynamic_lds_cache_key(int device, const void *kernel);

// (B*V, C, HW) -> (B*V, HW, C4), zero-padding channels C..C4; and the inverse for gradients
// (fp32 channels-last accumulator -> feature dtype, planar).
hipError_t launch_to_channels_last(const void *src, void *dst, const Problem &p, hipStream_t s);
hipError_t launch_grad_to_planar(const float *srcT, void *dst, const Problem &p, hipStream_t s);
// column-major quad-planar fp32 copy (MVHMR_LAYOUT_QUAD) -> channels-last in the feature dtype (gated like the gather kernels)
bool quad_to_channels_last_supported(const Problem &p);
hipError_t launch_quad_to_channels_last(const void *srcK, void *dst, const Problem &p, hipStream_t s);
// channels-last fp32 accumulator -> channels-last feature dtype (C4 == C required)
hipError_t launch_grad_cast(const float *srcT, void *dst, const Problem &p, hipStream_t s);

// gather variant: featT is channels-last (B,V,HW,C4) in the feature dtype
hipError_t launch_fwd_gather(const void *featT, const float *proj, const Coords &coords, void *out,
                             const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather(const void *grad_out, const void *featT, const float *proj, const Coords &coords,
                             float *gradT, const Problem &p, hipStream_t s);

// deterministic mode (unproject_det.hip, det_scale.h): the scale pass writes K[b][c] into `scale` (det_scale_bytes(p)) from grad_out and the
// channels-last feature copy; k_bwd_gather_det adds int64 fixed point into gradI (zeroed, channels-last (B,V,HW,C4)); the conversion passes
// write the caller's planar or channels-last gradient (NaN for a poisoned (b, c)).  One scale pass serves every family: what the bound
// ranges over is read off the problem (view_count, view_weights, visible, conf / confidence, feature_index / volumes, moments), the layout
// of `scale` off its route flags alone, so det_scale_bytes answers before any pointer exists, and det_exponents finds K in it.  feat is the
// channels-last copy, or the quad-planar one (quad: the plain route only); a call whose bound ranges over the tapped pixels (visible,
// confidence, moments) needs proj and coords
size_t det_scale_bytes(const Problem &p);
hipError_t launch_det_scale(const void *grad_out, const void *feat, void *scale, const Problem &p, hipStream_t s, bool quad = false,
                            const float *proj = nullptr, const Coords *coords = nullptr);
const int *det_exponents(const void *scale, const Problem &p);
hipError_t launch_bwd_gather_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                 const int *kexp, const Problem &p, hipStream_t s);
hipError_t launch_det_grad_to_planar(const unsigned long long *gradI, const int *kexp, void *dst, const Problem &p, hipStream_t s);
// brick kernels in deterministic mode: acc zeroed int64 quad-planar (B,V,C4/4,W,H,4); a smaller per-sample limit than brick_bwd_supported
bool brick_bwd_det_supported(const Problem &p);
hipError_t launch_bwd_brick_det(const void *featK, const void *grad_out, const float *proj, const Coords &coords, unsigned long long *acc,
                                const int *kexp, const Problem &p, hipStream_t s);
hipError_t launch_det_quad_to_planar(const unsigned long long *acc, const int *kexp, void *dst, const Problem &p, hipStream_t s);
hipError_t launch_det_grad_cast(const unsigned long long *gradI, const int *kexp, void *dst, const Problem &p, hipStream_t s);

// brick variant (LDS-staged windows); launches return hipErrorNotSupported when the shape does not qualify.
//   forward : column-major quad-planar staged copy (launch_to_quad_planar_t), 4*nvox x (NT/128) x 32 bricks
//   backward: the same column-major quad-planar staged copy, 8 x 8 x 16 (8 x 4 x 16 for 8 views) or 4 x (NT/128) x 32 bricks
bool brick_fwd_supported(const Problem &p);
bool brick_fwd_ws_shape(const Problem &p);      // the wave-specialised forward serves this problem
bool brick_fwd_prescales(const Problem &p);     // ... and wants its staged copy multiplied by log2(e): set Problem::feat_log2e for BOTH the layout pass and the kernel
bool brick_bwd_supported(const Problem &p);
size_t brick_workspace_bytes(const Problem &p);
hipError_t launch_to_quad_planar_t(const void *src, void *dst, const Problem &p, hipStream_t s, bool brick_side = true);
// the same copy from channels-last features (BV, H, W, C)
hipError_t launch_channels_last_to_quad_planar_t(const void *src, void *dst, const Problem &p, hipStream_t s);
hipError_t launch_fwd_brick(const void *featK, const float *proj, const Coords &coords, void *out, const Problem &p,
                            hipStream_t s);

// plane backward (unproject_plane_bwd.hip): the gradient plane of one (sample, view, channel quad) accumulated in LDS, no global
// atomics; the gather family's backward for planar / quad-planar features whose maps fit (Hf * (Wf | 1) * 16 B of LDS)
bool plane_bwd_supported(const Problem &p);
size_t plane_table_bytes(const Problem &p);
hipError_t launch_bwd_plane(const void *featK, const void *grad_out, const float *proj, const Coords &coords, void *grad_features,
                            void *table, const Problem &p, hipStream_t s);

// Geometry gate.  Counts the bricks whose pooled tap windows would not fit (from the projections of each brick's 8 corner
// voxels; speed heuristic only) into *count (zeroed by the caller).  GateGeom describes the bricks and windows of the kernel
// the gate decides for.
struct GateGeom {
    int bx, by, bz;      // brick extent in voxels
    int view_group;      // views whose windows are resident together (0: all of them)
    int column_major;    // window lines run along y (forward) or x (backward)
    int parity_rows;     // forward: the rows of a window column are split by parity (line stride 2 * ceil(rows / 2), origin row even)
    int cap_slots;       // 16-B LDS slots one window set may use
    int max_chunks;      // 64-slot DMA chunks a block can issue per quad
};
GateGeom brick_fwd_gate_geom(const Problem &p);
GateGeom brick_bwd_gate_geom(const Problem &p);
hipError_t launch_brick_gate(const float *proj, const Coords &coords, int *count, const GateGeom &g, const Problem &p, hipStream_t s);
int brick_count(const Problem &p, const GateGeom &g);

// brick backward: featK quad-planar features, gradK zeroed fp32 quad-planar accumulator (same shape)
hipError_t launch_bwd_brick(const void *featK, const void *grad_out, const float *proj, const Coords &coords, float *gradK,
                            const Problem &p, hipStream_t s);
hipError_t launch_quad_grad_to_planar(const float *gradK, void *dst, const Problem &p, hipStream_t s);

// process_feature fused with the layout pass: y = W x + b as an fp32 MFMA GEMM writing the column-major quad-planar copy
bool conv1x1_quad_supported(int Cin, int Cout, int H, int W);
bool conv1x1_planar_supported(int Cin, int Cout, int HW);
bool conv1x1_wgrad_supported(int Cin, int Cout, int HW);
hipError_t launch_conv1x1_wgrad(const float *gy, const float *x, float *dW, float *db, int BV, int Cin, int Cout, int HW, hipStream_t s);
// deterministic form: per-slice partial slabs in `ws` (conv1x1_wgrad_det_workspace_bytes), summed in a fixed order; dW / db are written
size_t conv1x1_wgrad_det_workspace_bytes(int BV, int Cin, int Cout, int HW);
hipError_t launch_conv1x1_wgrad_det(const float *gy, const float *x, float *dW, float *db, void *ws, int BV, int Cin, int Cout, int HW, hipStream_t s);
// the two below put the map index in the grid's z extent: BV <= kConv1x1MaxMaps, else hipErrorNotSupported.  All four GEMMs read x, w,
// bias and gy (and write the quad-planar dst) with 16-byte accesses: the C ABI checks the pointers
constexpr int kConv1x1MaxMaps = 65535;
hipError_t launch_conv1x1_planar(const float *x, const float *w, const float *bias, float *dst, int BV, int Cin, int Cout, int HW, hipStream_t s);
hipError_t launch_conv1x1_quad(const float *x, const float *w, const float *bias, void *dst, int BV, int Cin, int Cout, int H, int W,
                               hipStream_t s);

// DLT triangulation of one point per sample (fp32 in / out, float64 inside); points (V,2) shared or (B,V,2) per sample
hipError_t launch_triangulate_dlt(const float *proj, const float *points, const float *conf, float *out, int B, int V, int points_per_sample,
                                  int conf_per_sample, hipStream_t s);
// its backward: grad_out (B,3) -> grad_proj (B,V,3,4), grad_points (B,V,2), grad_conf (B,V), each per sample and each optional;
// NaN where the gradient does not exist (V < 2, a degenerate eigenvalue)
hipError_t launch_triangulate_dlt_bwd(const float *proj, const float *points, const float *conf, const float *grad_out, float *grad_proj,
                                      float *grad_points, float *grad_conf, int B, int V, int points_per_sample, int conf_per_sample, hipStream_t s);

// gradient w.r.t. proj and coords (unproject_geom_bwd.hip): featT channels-last (B,V,HW,C4) in the feature dtype; `part` holds
// geom_partial_bytes(p) of fp32 partials of grad_proj (needed when grad_proj is non-null); either output may be null
size_t geom_partial_bytes(const Problem &p);
// per-view weights (Problem::view_weights): grad_weights (B, V) fp32 in SLOT order from wpart (geom_weight_partial_bytes(p) of fp32
// partials), both null when not asked for; it may be the only output
size_t geom_weight_partial_bytes(const Problem &p);
// (the weighted instances of k_bwd_geom live in unproject_geom_bwd_weighted.hip; launch_bwd_geom[_cuboid] call this for them)
hipError_t launch_bwd_geom_weighted_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                           float *grad_coords, float *pose_part, float *wpart, bool pose, const Problem &p, hipStream_t s);
hipError_t launch_bwd_geom(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                           float *grad_coords, const Problem &p, hipStream_t s, float *wpart = nullptr, float *grad_weights = nullptr);
// the same for the cuboid recipe (coords.ptr == null): grad_proj as above, and the gradients w.r.t. the pose, grad_rot (B,3,3) and
// grad_center (B,3), from pose_part (pose_partial_bytes(p) of fp32 partials, needed when either is non-null); grad_coords is not written
size_t pose_partial_bytes(const Problem &p);
hipError_t launch_bwd_geom_cuboid(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                                  float *pose_part, float *grad_rot, float *grad_center, const Problem &p, hipStream_t s, float *wpart = nullptr,
                                  float *grad_weights = nullptr);

// visibility-aware aggregation (unproject_visible.hip; Problem::visible): the gather forward, the per-tap scatter backward of both modes
// (launch_fwd_gather / launch_bwd_gather / launch_bwd_gather_det call these for visible problems), and the bitmask itself -- bits (B, N)
// int32, bit v = view v is present (mask (B, V) bytes, null: all) and sees the voxel
hipError_t launch_fwd_gather_seen(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather_seen(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s);
hipError_t launch_bwd_gather_seen_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s);
hipError_t launch_view_visibility(const float *proj, const Coords &coords, const uint8_t *mask, int *bits, const Problem &p, hipStream_t s);
// (the seen instances of k_bwd_geom live in unproject_visible_geom.hip; launch_bwd_geom[_cuboid] call this for visible problems)
hipError_t launch_bwd_geom_seen_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                       float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s);

// per-pixel view confidence (unproject_confidence.hip; Problem::confidence): the gather forward and the per-tap scatter backward of both modes
// (launch_fwd_gather / launch_bwd_gather / launch_bwd_gather_det call these for confidence problems; the deterministic scale pass is
// launch_det_scale's, whose bound carries the sample's largest confidence pixel), and grad_confidence (B, V, Hf, Wf) fp32 from the
// geometry kernel's stream: bitwise reproducible, integer atomics only, every element written
hipError_t launch_fwd_gather_conf(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather_conf(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s);
hipError_t launch_bwd_gather_conf_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s);
size_t conf_grad_stream_bytes(const Problem &p);
size_t conf_grad_acc_bytes(const Problem &p);
size_t conf_grad_max_bytes(const Problem &p);
hipError_t launch_conf_grad(const float *stream, const float *proj, const Coords &coords, unsigned long long *acc, unsigned *smax, float *grad_conf,
                            const Problem &p, hipStream_t s);
// (the confidence instances of k_bwd_geom live in unproject_confidence_geom.hip; launch_bwd_geom[_cuboid] call this for confidence problems)
hipError_t launch_bwd_geom_conf_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                       float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s);

// shared feature maps (unproject_shared.hip, unproject_shared_geom.hip; Problem::feature_index / volumes): the gather forward, the per-tap scatter
// backward of both modes (launch_det_scale's exponents are per FEATURE sample and channel, and carry cnt[b], the number of volumes that name b)
// and the geometry backward, whose grad_proj and pose partials are per VOLUME (shared_geom_partial_bytes / shared_pose_partial_bytes) and are
// summed per (b, v) over the volumes that name b in ascending order.  The volume index is the grid's y extent.
constexpr int kSharedMaxVolumes = 65535;
hipError_t launch_fwd_gather_shared(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather_shared(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                    hipStream_t s);
hipError_t launch_bwd_gather_shared_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                        const int *kexp, const Problem &p, hipStream_t s);
size_t shared_geom_partial_bytes(const Problem &p);
size_t shared_pose_partial_bytes(const Problem &p);
hipError_t launch_bwd_geom_shared(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                                  float *grad_coords, const Problem &p, hipStream_t s);
hipError_t launch_bwd_geom_cuboid_shared(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                                         float *pose_part, float *grad_rot, float *grad_center, const Problem &p, hipStream_t s);

// lens distortion (unproject_lens.hip, unproject_lens_geom.hip; Problem::lens): the gather forward, the per-tap scatter backward of both modes (the
// deterministic scale pass is the plain one: its bound does not depend on where the taps land), the plane backward's tap table (launch_bwd_plane
// calls it for a lens problem; tabW is its float4 table) and the lens instances of k_bwd_geom (launch_bwd_geom[_cuboid] call this for them)
hipError_t launch_fwd_gather_lens(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather_lens(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s);
hipError_t launch_bwd_gather_lens_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s);
hipError_t launch_plane_taps_lens(const float *proj, const Coords &coords, void *tabW, int *tabX, int *cmax, const Problem &p, hipStream_t s);
hipError_t launch_bwd_geom_lens_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                       float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s);

// cross-view variance (unproject_moments.hip, unproject_moments_geom.hip; Problem::moments): the gather forward, the per-tap scatter backward of
// both modes (launch_det_scale's bound carries both halves of grad_out and the largest feature a participating view taps) and the moments
// instances of k_bwd_geom (launch_bwd_geom[_cuboid] call this for them).  out / grad_out hold moments * C channels.
hipError_t launch_fwd_gather_moments(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s);
hipError_t launch_bwd_gather_moments(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                     hipStream_t s);
hipError_t launch_bwd_gather_moments_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                         const int *kexp, const Problem &p, hipStream_t s);
hipError_t launch_bwd_geom_moments_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                          float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s);

// view masks (view_mask.hip): from mask (B,V) bytes, one thread per sample writes n_b (B ints), slot -> view and view -> slot (-1: masked)
// tables (B,V ints each) and the projections packed into slot order (absent slots zero); then per-(sample, slot) copies of `bytes_per_view`
// bytes in and out of slot order: pack (absent slots zero-filled) and unpack (masked views zero-filled)
size_t view_table_bytes(int B, int V);
hipError_t launch_view_table(const uint8_t *mask, const float *proj, void *table, int B, int V, hipStream_t s);
const int *view_table_counts(const void *table);
const float *view_table_proj(const void *table, int B, int V);
// per-view weights: presence = mask (null: all) and weight > 0; the table as above, then the weights packed into slot order (absent slots 0)
size_t weighted_view_table_bytes(int B, int V);
hipError_t launch_view_table_weighted(const uint8_t *mask, const float *weights, const float *proj, void *table, int B, int V, hipStream_t s);
const float *view_table_weights(const void *table, int B, int V);
hipError_t launch_view_pack(const void *src, void *dst, const void *table, int B, int V, size_t bytes_per_view, hipStream_t s);
hipError_t launch_view_unpack(const void *src, void *dst, const void *table, int B, int V, size_t bytes_per_view, hipStream_t s);

hipError_t launch_build_coords(float *coords_out, const float *rot, const float *center, int B, int S,
                               const double pos[3], const double sides[3], hipStream_t s);

// volumetric soft-argmax (soft_argmax3d.hip).  `dtype` is an mvhmr_dtype_t of vol / grad_vol; coords.ptr selects the tensor
// route, else the cuboid recipe; c2 = fl32(beta * log2 e).  ws holds sa3d_workspace_floats(B, J, N) floats of per-split records.
int sa3d_splits(long long B, long long J, long long N);
size_t sa3d_workspace_floats(long long B, long long J, long long N);
hipError_t launch_sa3d_forward(const void *vol, int dtype, const Coords &coords, int B, int J, int X, float c2, float *keypoints, float *lse,
                               float *moment, float *ws, hipStream_t s);
hipError_t launch_sa3d_backward(const void *vol, int dtype, const Coords &coords, int B, int J, int X, float c2, float beta, const float *lse,
                                const float *moment, const float *grad_kp, const float *grad_lse, void *grad_vol, hipStream_t s);
hipError_t launch_sa3d_backward_coords(const void *vol, int dtype, int B, int J, long long N, float c2, const float *lse, const float *grad_kp,
                                       float *grad_coords, hipStream_t s);
hipError_t launch_sa3d_backward_pose(const float *rot, const float *moment, const float *grad_kp, float *grad_rot, float *grad_center, int B, int J,
                                     hipStream_t s);

// trilinear volume sampling at world points (volume_sample.hip).  `dtype` is an mvhmr_dtype_t of vol / grad_vol; cs is the
// cuboid recipe (never a tensor); index (B,N,3) is the forward's continuous voxel index, which both backwards read.  ws holds
// vs3d_workspace_bytes(B, N) bytes: the sorted tap tables of the volume gradient, or the (B,N,3) per-point u of the geometry gradient.
int vs3d_chunk_points();
size_t vs3d_workspace_bytes(long long B, long long N);
hipError_t launch_vs3d_forward(const void *vol, int dtype, const Coords &cs, const float *points, int B, int C, int X, int N, int paired,
                               float *samples, float *index, hipStream_t s);
hipError_t launch_vs3d_backward_volumes(int dtype, const float *index, const float *grad_samples, int B, int C, int X, int Y, int Z, int N, int paired,
                                        void *grad_vol, void *ws, hipStream_t s);
hipError_t launch_vs3d_backward_geometry(const void *vol, int dtype, const Coords &cs, const float *points, const float *index, const float *grad_samples,
                                         int B, int C, int X, int N, int paired, float *grad_points, float *grad_rot, float *grad_center, float *ws,
                                         hipStream_t s);

// 3-D non-maximum suppression and top-K (volume_peaks.hip).  `dtype` is an mvhmr_dtype_t of vol / grad_vol; cs is the cuboid
// recipe and is read only when positions is non-null.  ws holds pk3d_workspace_bytes(...) bytes: pk3d_blocks_per_slice * K keys per slice.
// tkey is the order-preserving key of the threshold (pk3d_key).
void pk3d_tile(int tile[3]);
int pk3d_max_k();
unsigned pk3d_key(float v);
long long pk3d_blocks_per_slice(int X, int Y, int Z);
size_t pk3d_workspace_bytes(long long B, long long J, int X, int Y, int Z, int K);
hipError_t launch_pk3d_forward(const void *vol, int dtype, const Coords &cs, int B, int J, int X, int Y, int Z, int K, int radius, unsigned tkey,
                               float *scores, int *index, float *positions, void *ws, hipStream_t s);
hipError_t launch_pk3d_backward(int dtype, const int *index, const float *grad_scores, long long slices, long long N, int K, void *grad_vol,
                                hipStream_t s);
hipError_t launch_pk3d_backward_pose(const int *index, const float *grad_pos, const Coords &cs, int B, int J, int K, float *grad_rot,
                                     float *grad_center, hipStream_t s);

// ray-marching volumes into camera-view maps (volume_project.hip).  `dtype` is an mvhmr_dtype_t of vol / grad_vol, `method` an
// mvhmr_project_t; cs is the cuboid recipe; rays (B,V,3,4).  aux: the arg-k (max) or the log-sum-exp (softmax) per map element.  ws holds
// pv3d_workspace_bytes(B, C, X*Y*Z) bytes: the scale tables and the int64 accumulator of pv3d_pass_channels(...) channels.
int pv3d_max_samples();
void pv3d_channel_group(int group_unroll[2]);
int pv3d_pass_channels(long long B, long long C, long long vox);
size_t pv3d_workspace_bytes(long long B, long long C, long long vox);
hipError_t launch_pv3d_forward(const void *vol, int dtype, const Coords &cs, const float *rays, int B, int V, int C, int X, int Hm, int Wm, int K,
                               int method, float beta, float dmin, float dmax, float *maps, float *ranges, void *aux, hipStream_t s);
hipError_t launch_pv3d_backward_volumes(const void *vol, int dtype, const Coords &cs, const float *rays, int B, int V, int C, int X, int Hm, int Wm,
                                        int K, int method, float beta, float dmin, float dmax, const float *grad_maps, const float *maps,
                                        const void *aux, void *grad_vol, void *ws, hipStream_t s);

}  // namespace mvhmr
