// extern "C" surface of libmvhmr_unproject.so -- see include/mvhmr_unproject.h for the contract and the
// reference interface (models/aggregation.py:20-87) each entry point replaces.
#include "mvhmr_unproject.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <cmath>
#include <mutex>
#include <unordered_map>

#include "device_common.h"
#include "kernels.h"

using namespace mvhmr;

namespace mvhmr {
unsigned long long dynamic_lds_cache_key(int device, const void *kernel)
{
    // kernel entry points are at least 256-B aligned, so the low byte of the pointer is free for the device ordinal
    return (unsigned long long)reinterpret_cast<uintptr_t>(kernel) ^ ((unsigned long long)(unsigned)device << 56) ^ (unsigned long long)(device & 0xff);
}

hipError_t allow_dynamic_lds(const void *kernel, size_t bytes)
{
    static std::mutex mu;
    static std::unordered_map<unsigned long long, size_t> granted;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long key = dynamic_lds_cache_key(dev, kernel);
    std::lock_guard<std::mutex> lock(mu);
    auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) granted[key] = bytes;
    return e;
}
}  // namespace mvhmr

namespace {

thread_local char g_err[512] = "";

int fail(int status, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return status;
}

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int check_desc(const mvhmr_unproject_desc *d, Problem *p)
{
    if (!d) return fail(MVHMR_ERR_INVALID_ARGUMENT, "descriptor is null");
    if (d->abi_version != MVHMR_ABI_VERSION)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "descriptor abi_version %d, library speaks %d", d->abi_version, MVHMR_ABI_VERSION);
    if (d->batch < 1 || d->views < 1 || d->channels < 1 || d->feat_h < 1 || d->feat_w < 1 || d->vol_x < 1 || d->vol_y < 1 || d->vol_z < 1)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "every dimension must be >= 1 (B=%d V=%d C=%d Hf=%d Wf=%d vol=%dx%dx%d)", d->batch, d->views,
                    d->channels, d->feat_h, d->feat_w, d->vol_x, d->vol_y, d->vol_z);
    if (d->method < MVHMR_AGG_SOFTMAX || d->method > MVHMR_AGG_MAX)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "Unknown aggregation_method: %d", d->method);
    if (d->feat_dtype < 0 || d->feat_dtype > MVHMR_BF16 || d->out_dtype < 0 || d->out_dtype > MVHMR_BF16)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown dtype (feat %d, out %d)", d->feat_dtype, d->out_dtype);
    if (d->feat_dtype == MVHMR_BF16)
        return fail(MVHMR_ERR_UNSUPPORTED, "bf16 is a storage type of the volume only (out_dtype); features are fp32 or fp16");
    if (d->out_dtype == MVHMR_BF16 && d->feat_dtype != MVHMR_F32)
        return fail(MVHMR_ERR_UNSUPPORTED, "a bf16 volume needs fp32 features");
    if (d->feat_layout < 0 || d->feat_layout > MVHMR_LAYOUT_QUAD_LOG2E) return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown feature layout %d", d->feat_layout);
    if (d->variant < 0 || d->variant > MVHMR_VARIANT_BRICK) return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown kernel variant %d", d->variant);
    if (d->views > kMaxViews) return fail(MVHMR_ERR_UNSUPPORTED, "at most %d views are supported (got %d)", kMaxViews, d->views);
    if (d->feat_dtype == MVHMR_F32 && d->out_dtype == MVHMR_F16)
        return fail(MVHMR_ERR_UNSUPPORTED, "fp32 features with an fp16 volume is not a supported storage mode");
    p->B = d->batch; p->V = d->views; p->C = d->channels; p->H = d->feat_h; p->W = d->feat_w;
    p->X = d->vol_x; p->Y = d->vol_y; p->Z = d->vol_z;
    p->N = (long long)d->vol_x * d->vol_y * d->vol_z;
    p->C4 = (d->channels + 3) / 4 * 4;
    p->method = d->method;
    p->feat_f16 = d->feat_dtype == MVHMR_F16;
    p->out_f16 = d->out_dtype == MVHMR_F16;
    p->out_bf16 = d->out_dtype == MVHMR_BF16;
    if ((long long)p->H * p->W * p->C4 >= (1ll << 31))
        return fail(MVHMR_ERR_UNSUPPORTED, "one feature map (Hf*Wf*C = %lld elements) exceeds 32-bit tap offsets", (long long)p->H * p->W * p->C4);
    if (d->feat_layout == MVHMR_LAYOUT_BVHWC && p->C4 != p->C)
        return fail(MVHMR_ERR_UNSUPPORTED, "channels-last features need C %% 4 == 0 (C = %d)", p->C);
    // (quad-planar copies hold (C + 3) / 4 quads per view, the last one zero-padded: any C the brick kernels take)
    return MVHMR_OK;
}

size_t feat_elem(const Problem &p) { return p.feat_f16 ? 2 : 4; }
size_t featT_bytes(const Problem &p) { return align_up((size_t)p.B * p.V * p.H * p.W * p.C4 * feat_elem(p)); }
size_t gradT_bytes(const Problem &p) { return align_up((size_t)p.B * p.V * p.H * p.W * p.C4 * sizeof(float)); }

constexpr int kChipCUs = 256;       // MI355X

// AUTO prefers the brick forward only when the launch holds enough voxels to keep the chip busy: every block walks all C / 4 quads
// whatever the volume, so one round of bricks costs the same run time however few of them there are, while the gather kernels' time
// falls with the voxel count.  Measured break-even (profiles/r04_configs/brick_count_sweep.txt: 16^3 ... 32^3 grids, 32 ... 256
// channels, 12 ... 96 px maps): between 64 and 108 bricks' worth of voxels; the reference's shipped 16^3 x 32 samples (64 bricks' worth,
// half of every brick past the volume's top) runs 0.13 ms on the gather kernels against 0.21 ms.  variant = brick still forces the bricks.
constexpr long long kBrickFwdMinVoxels = 96ll * 8 * 8 * 32;             // 96 bricks of 8 x 8 x 32
bool brick_fwd_preferred(const Problem &p)
{
    return brick_fwd_supported(p) && static_cast<long long>(p.B) * p.X * p.Y * p.Z >= kBrickFwdMinVoxels;
}

// which kernel runs: channels-last input feeds the gather kernels; quad-planar input (the fused 1x1 conv's output) the brick kernels,
// or -- through one more layout pass -- the gather kernels when the caller or the shape asks for them
int pick_variant(const mvhmr_unproject_desc *d, const Problem &p)
{
    if (d->feat_layout == MVHMR_LAYOUT_BVHWC) return MVHMR_VARIANT_GATHER;
    if (d->variant != MVHMR_VARIANT_AUTO) return d->variant;
    return brick_fwd_preferred(p) ? MVHMR_VARIANT_BRICK : MVHMR_VARIANT_GATHER;
}

int variant_conflict(const mvhmr_unproject_desc *d, const Problem &p, int variant)
{
    if (variant == MVHMR_VARIANT_BRICK && !brick_fwd_supported(p)) return fail(MVHMR_ERR_UNSUPPORTED, "the brick variant does not support this shape / dtype");
    if (d->variant != MVHMR_VARIANT_AUTO && d->variant != variant)
        return fail(MVHMR_ERR_UNSUPPORTED, "feature layout %d cannot feed kernel variant %d", d->feat_layout, d->variant);
    if (variant == MVHMR_VARIANT_GATHER && d->feat_layout == MVHMR_LAYOUT_QUAD && !quad_to_channels_last_supported(p))
        return fail(MVHMR_ERR_UNSUPPORTED, "quad-planar features of this shape cannot feed the gather kernels (C <= 4092, B * V <= 65535)");
    return MVHMR_OK;
}

// the gradient can be accumulated straight into grad_features when that already is fp32 channels-last
bool grad_in_place(const mvhmr_unproject_desc *d, const Problem &p) { return d->feat_layout == MVHMR_LAYOUT_BVHWC && !p.feat_f16; }

// The brick backward (window gradients accumulated in LDS in fixed point, then flushed with 256-B shaped float atomics)
// is the default wherever the brick forward is: ~20 GB of global atomic traffic instead of the gather backward's 137 GB
// (17 ms against 104 ms at the north-star size: profiles/r01_final_pmc.txt).  variant = gather keeps the gather backward.
bool bwd_uses_brick(const mvhmr_unproject_desc *d, const Problem &p)
{
    if (d->feat_layout == MVHMR_LAYOUT_QUAD && p.feat_f16) return false;        // the quad copy is fp32; mixed storage goes through the gather backward
    // A volume of fewer bricks than the chip has CUs (the reference's shipped 16^3: 4 bricks per sample) leaves most of it idle while every
    // block still walks all C / 4 quads: 0.48 ms for 32 samples of 16^3 against 0.2x for the plane kernels, whose blocks are (sample,
    // view, quad).  AUTO then takes the plane backward; variant = brick still forces the bricks.
    if (d->variant == MVHMR_VARIANT_AUTO && plane_bwd_supported(p) && brick_bwd_supported(p) && brick_count(p, brick_bwd_gate_geom(p)) < kChipCUs) return false;
    return (d->feat_layout == MVHMR_LAYOUT_BVCHW || d->feat_layout == MVHMR_LAYOUT_QUAD) && d->variant != MVHMR_VARIANT_GATHER && brick_bwd_supported(p);
}

// The gather family's backward for planar / quad-planar features: the plane kernel (no global atomics) where the maps fit LDS, else
// the per-tap scatter.  Channels-last features keep the scatter (its accumulator is the caller's own tensor).
bool bwd_uses_plane(const mvhmr_unproject_desc *d, const Problem &p)
{
    return d->feat_layout != MVHMR_LAYOUT_BVHWC && plane_bwd_supported(p) && !p.masked;   // (masked calls: the per-tap scatter)
}
// bytes between the converted feature copy and the gate counter of a gated backward: the brick side's accumulator or the plane
// side's tap table, whichever is larger
size_t bwd_mid_bytes(const mvhmr_unproject_desc *d, const Problem &p)
{
    const size_t a = gradT_bytes(p), b = bwd_uses_plane(d, p) ? align_up(plane_table_bytes(p)) : 0;
    return a > b ? a : b;
}

// AUTO on planar input, for a shape both variants serve: the variant is chosen on the device from the geometry (gate.h).
// Quad-planar input is gated the same way (the gather side then converts it to channels-last first), so a caller that keeps
// only the fused conv's copy never pins a variant the geometry does not suit.
bool gateable_layout(const mvhmr_unproject_desc *d, const Problem &p)
{
    return d->feat_layout == MVHMR_LAYOUT_BVCHW || (d->feat_layout == MVHMR_LAYOUT_QUAD && quad_to_channels_last_supported(p));
}
bool geometry_gated(const mvhmr_unproject_desc *d, const Problem &p)
{
    return d->variant == MVHMR_VARIANT_AUTO && gateable_layout(d, p) && brick_fwd_preferred(p);
}
// the backward has its own bricks and windows, hence its own gate
bool geometry_gated_bwd(const mvhmr_unproject_desc *d, const Problem &p)
{
    return d->variant == MVHMR_VARIANT_AUTO && gateable_layout(d, p) && brick_bwd_supported(p);
}
constexpr size_t kGateBytes = 256;
// the converted feature copy of a gated launch: channels-last in the feature dtype or quad-planar fp32, whichever is larger
size_t conv_bytes(const Problem &p) { const size_t a = featT_bytes(p), b = brick_workspace_bytes(p); return a > b ? a : b; }

// zeroes the counter at the end of the workspace region `at`, counts the overflowing bricks, arms the gate in p
int arm_gate(Problem &p, unsigned char *at, const float *proj, const Coords &coords, const GateGeom &g, hipStream_t s)
{
    int *count = reinterpret_cast<int *>(at);
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    if (e != hipSuccess) return fail(MVHMR_ERR_LAUNCH, "geometry gate clear: %s", hipGetErrorString(e));
    e = launch_brick_gate(proj, coords, count, g, p, s);
    if (e != hipSuccess) return fail(MVHMR_ERR_LAUNCH, "geometry gate: %s", hipGetErrorString(e));
    p.gate_count = count;
    p.gate_limit = brick_count(p, g) / 8;       // brick variant while at most 1/8 of the bricks would take its slow path
    return MVHMR_OK;
}

int check_ws(void *ws, size_t have, size_t need)
{
    if (need == 0) return MVHMR_OK;
    if (!ws) return fail(MVHMR_ERR_WORKSPACE, "workspace is null but %zu bytes are required", need);
    if (have < need) return fail(MVHMR_ERR_WORKSPACE, "workspace has %zu bytes, %zu are required", have, need);
    if (reinterpret_cast<uintptr_t>(ws) % kAlign) return fail(MVHMR_ERR_WORKSPACE, "workspace must be %zu-byte aligned", kAlign);
    return MVHMR_OK;
}

Coords coords_from_tensor(const float *coords, const Problem &p)
{
    Coords c{};
    c.ptr = coords; c.Y = p.Y; c.Z = p.Z;
    return c;
}

// the reference's cuboid recipe (aggregation.py:140-187): corner `position`, edge lengths `sides` (float64 on the host, cast to
// fp32 when they meet the tensor), per-sample rotation and pivot on the device
int coords_from_cuboid(const float *rot, const float *center, const double position[3], const double sides[3], const Problem &p, Coords *out)
{
    if (!rot || !center || !position || !sides) return fail(MVHMR_ERR_INVALID_ARGUMENT, "rot / center / position / sides must be non-null");
    Coords c{};
    c.ptr = nullptr; c.rot = rot; c.center = center; c.Y = p.Y; c.Z = p.Z;
    c.px = (float)position[0]; c.py = (float)position[1]; c.pz = (float)position[2];
    // step = sides / (S - 1) in float64, then fp32 (aggregation.py:157-159); a one-voxel axis has no step
    c.sx = p.X > 1 ? (float)(sides[0] / (double)(p.X - 1)) : 0.f;
    c.sy = p.Y > 1 ? (float)(sides[1] / (double)(p.Y - 1)) : 0.f;
    c.sz = p.Z > 1 ? (float)(sides[2] / (double)(p.Z - 1)) : 0.f;
    *out = c;
    return MVHMR_OK;
}

int launched(hipError_t e, const char *what)
{
    if (e == hipSuccess) return MVHMR_OK;
    if (e == hipErrorNotSupported) return fail(MVHMR_ERR_UNSUPPORTED, "%s: no kernel for this dtype/shape combination", what);
    return fail(MVHMR_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

size_t max_size(size_t a, size_t b) { return a > b ? a : b; }

// ---- opening a call: what places the volume is either the coordinate tensor or the cuboid recipe
struct VolumeSource {
    const float *coords;                        // tensor form
    const float *rot, *center;                  // cuboid form
    const double *position, *sides;
    bool cuboid;
};
VolumeSource tensor_volume(const float *coords) { return VolumeSource{coords, nullptr, nullptr, nullptr, nullptr, false}; }
VolumeSource cuboid_volume(const float *rot, const float *center, const double position[3], const double sides[3])
{
    return VolumeSource{nullptr, rot, center, position, sides, true};
}

int make_coords(const VolumeSource &v, const Problem &p, Coords *out)
{
    if (v.cuboid) return coords_from_cuboid(v.rot, v.center, v.position, v.sides, p, out);
    if (!v.coords) return fail(MVHMR_ERR_INVALID_ARGUMENT, "coords must be non-null");
    *out = coords_from_tensor(v.coords, p);
    return MVHMR_OK;
}

// the descriptor, then the volume: every forward and feature-backward entry point starts here
int open_call(const mvhmr_unproject_desc *desc, const VolumeSource &v, Problem *p, Coords *coords)
{
    const int rc = check_desc(desc, p);
    return rc != MVHMR_OK ? rc : make_coords(v, *p, coords);
}

// ---- the call record (include/mvhmr_unproject.h): what an entry point's name and arguments say, as the routes read it.
// The rule of the families is written here once.  The view selections (mask, weights, seeing test, confidence maps, moments) select the
// packed route of the families that take them; a shared or lens record carries them only to be refused (shared_refused, lens_refused).
using Call = mvhmr_unproject_call;
VolumeSource placing_of(const Call &c)
{
    return c.placing == MVHMR_PLACING_CUBOID ? cuboid_volume(c.rot, c.center, c.position, c.sides) : tensor_volume(c.coords);
}
bool selects_views(const Call &c) { return c.family != MVHMR_FAMILY_SHARED && c.family != MVHMR_FAMILY_LENS; }
const uint8_t *mask_of(const Call &c) { return selects_views(c) ? c.view_mask : nullptr; }                // null: packs nothing
const float *weights_of(const Call &c) { return selects_views(c) ? c.view_weights : nullptr; }            // null: the masked (or plain) call
const float *confidence_of(const Call &c) { return selects_views(c) ? c.view_confidence : nullptr; }      // null: the visible or masked call
bool seeing(const Call &c) { return c.family == MVHMR_FAMILY_VISIBLE || (selects_views(c) && c.visible); }  // a visible call: always
int moments_of(const Call &c) { return c.family != MVHMR_FAMILY_MOMENTS ? 0 : c.moments ? c.moments : -1; }  // 0: refused as any other unknown value
bool packed(const Call &c) { return mask_of(c) || weights_of(c); }
// the optional inputs each family takes: a record that sets another one says what no named call can, and is refused
enum : unsigned { kMask = 1, kWeights = 2, kConfidence = 4, kVisible = 8, kIndex = 16, kLens = 32, kMoments = 64 };
constexpr unsigned kTakes[] = {0,                                                   // plain
                               kMask,                                               // masked
                               kMask | kWeights,                                    // weighted
                               kMask | kVisible,                                    // visible (the seeing test is on whatever the flag says)
                               kMask | kConfidence | kVisible,                      // confidence
                               kIndex | kMask | kWeights | kConfidence | kVisible,  // shared (the last four: refused with their own texts)
                               kLens | kMask | kWeights | kConfidence | kVisible | kIndex,     // lens (the last five likewise)
                               kMask | kVisible | kMoments};                        // moments
// struct_size, family and placing: what the workspace query checks too
int check_record(const Call *c)
{
    if (!c) return fail(MVHMR_ERR_INVALID_ARGUMENT, "call record is null");
    if (c->struct_size != sizeof(Call))
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "call record struct_size %u, library expects %zu", c->struct_size, sizeof(Call));
    if (c->family < MVHMR_FAMILY_PLAIN || c->family > MVHMR_FAMILY_MOMENTS) return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown call family %d", c->family);
    if (c->placing != MVHMR_PLACING_TENSOR && c->placing != MVHMR_PLACING_CUBOID) return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown placing %d", c->placing);
    return MVHMR_OK;
}
int check_call(const Call *c)
{
    if (const int rc = check_record(c)) return rc;
    const unsigned set = (c->view_mask ? kMask : 0) | (c->view_weights ? kWeights : 0) | (c->view_confidence ? kConfidence : 0) | (c->visible ? kVisible : 0) |
                         (c->feature_index ? kIndex : 0) | (c->lens ? kLens : 0) | (c->moments ? kMoments : 0);
    if (set & ~kTakes[c->family])
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "call family %d takes none of the optional inputs 0x%x the record sets (mask 1, weights 2, confidence 4, visible 8, "
                                                "feature_index 16, lens 32, moments 64)", c->family, set & ~kTakes[c->family]);
    return MVHMR_OK;
}

// ---- per-sample view masks (include/mvhmr_unproject.h).  k_view_table turns the mask into slot tables and the projections
// packed into slot order, the features are packed the same way (absent slots zero), and the unmasked route runs on the packed problem with
// Problem::view_count set: the gather family (forward, per-tap scatter backward, its deterministic form) and the geometry kernels.  Gradients
// are unpacked back into view order, masked views zero-filled.  A null mask is the unmasked call.
int mask_refused(const mvhmr_unproject_desc *desc)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "a view mask needs planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK) return fail(MVHMR_ERR_UNSUPPORTED, "a view mask runs the gather kernels: MVHMR_VARIANT_BRICK is not served");
    return MVHMR_OK;
}
// ---- per-view confidence weights (include/mvhmr_unproject.h): the packed route of the masks -- presence is mask && weight > 0,
// the weights are packed into slot order beside the projections (Problem::view_weights) and the gather / geometry kernels launch their
// weighted instances.  Null weights are the masked (or unmasked) call.  Refused where a mask is, and for max, which has no weighted form.
int weights_refused(const mvhmr_unproject_desc *desc)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "view weights need planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK) return fail(MVHMR_ERR_UNSUPPORTED, "view weights run the gather kernels: MVHMR_VARIANT_BRICK is not served");
    if (desc->method == MVHMR_AGG_MAX) return fail(MVHMR_ERR_UNSUPPORTED, "aggregation method max has no weighted form: pass a view mask instead of view weights");
    return MVHMR_OK;
}
// ---- visibility-aware aggregation (include/mvhmr_unproject.h): every voxel aggregates only the views that see it.  The
// route of the masks: the gather family with the per-tap scatter backward and the geometry kernels, which launch their *_seen kernels
// (Problem::visible); with a mask the views are packed exactly as for a masked call, without one nothing is packed or copied.  Refused
// where a mask is.
int visible_refused(const mvhmr_unproject_desc *desc)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "visibility-aware aggregation needs planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK)
        return fail(MVHMR_ERR_UNSUPPORTED, "visibility-aware aggregation runs the gather kernels: MVHMR_VARIANT_BRICK is not served");
    return MVHMR_OK;
}
// ---- per-pixel view confidence maps (include/mvhmr_unproject.h): the route of the visible calls -- the gather family with the
// per-tap scatter backward and the geometry kernels, which launch their *_conf kernels (Problem::confidence); with a mask the maps are packed
// in slot order together with the features, without one nothing is packed or copied.  Refused where weights are.
int confidence_refused(const mvhmr_unproject_desc *desc)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "view confidence maps need planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK)
        return fail(MVHMR_ERR_UNSUPPORTED, "view confidence maps run the gather kernels: MVHMR_VARIANT_BRICK is not served");
    if (desc->method == MVHMR_AGG_MAX)
        return fail(MVHMR_ERR_UNSUPPORTED, "aggregation method max has no weighted form: pass a view mask instead of view confidence maps");
    return MVHMR_OK;
}
// ---- shared feature maps (include/mvhmr_unproject.h): `volumes` volumes read the desc->batch feature samples through a device
// index.  The route of the masked calls without their head -- nothing is packed or copied: the gather family with the per-tap scatter backward
// and the geometry kernels, which launch their *_shared kernels (Problem::feature_index).  Every feature-sized region stays sized by the
// batch; only the geometry partials are per volume.  Refused where a mask is; the view selections (mask, weights, seeing test, confidence
// maps) do not compose with the index yet and are refused each with its own text.  A null index with volumes == batch is the plain gather call.
// the checks that need no index: what the workspace queries ask too
int shared_shape_refused(const mvhmr_unproject_desc *desc, int32_t volumes)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "shared feature maps need planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK) return fail(MVHMR_ERR_UNSUPPORTED, "shared feature maps run the gather kernels: MVHMR_VARIANT_BRICK is not served");
    if (volumes < 1) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volumes must be >= 1 (got %d)", volumes);
    if (volumes > kSharedMaxVolumes)
        return fail(MVHMR_ERR_UNSUPPORTED, "at most %d volumes per call (the volume index is the grid's y extent; got %d): split the call", kSharedMaxVolumes, volumes);
    return MVHMR_OK;
}
int shared_refused(const mvhmr_unproject_desc *desc, const Call &c)
{
    if (c.view_mask) return fail(MVHMR_ERR_UNSUPPORTED, "feature_index with a view mask is not built yet: un-project the masked samples on their own");
    if (c.view_weights) return fail(MVHMR_ERR_UNSUPPORTED, "feature_index with view weights is not built yet: un-project the weighted samples on their own");
    if (c.visible) return fail(MVHMR_ERR_UNSUPPORTED, "feature_index with visibility-aware aggregation is not built yet: un-project those samples on their own");
    if (c.view_confidence) return fail(MVHMR_ERR_UNSUPPORTED, "feature_index with view confidence maps is not built yet: un-project those samples on their own");
    if (const int rc = shared_shape_refused(desc, c.volumes)) return rc;
    if (!c.feature_index && c.volumes != desc->batch)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "a null feature_index is the plain call: volumes (%d) must equal batch (%d)", c.volumes, desc->batch);
    return MVHMR_OK;
}
// ---- lens distortion (include/mvhmr_unproject.h): one Brown-Conrady record per (sample, view) through which the voxels are
// projected.  The plain gather route with the gather variant -- forward, the plane backward wherever the plain gather call takes it (its tap
// table is built through the records), else the per-tap scatter, both modes, and the geometry kernels -- whose launchers hand a problem with
// Problem::lens to the *_lens kernels.  Nothing is packed or copied, no region is added.  The brick variant and the quad-planar layouts are
// refused (a brick's window is bounded by the projective image of its corners, which does not hold under distortion); the view selections and
// the feature index do not compose with the lens yet and are refused each with its own text.  A null lens is the plain gather call.
// the checks that need no pointer: what the workspace queries ask too
int lens_shape_refused(const mvhmr_unproject_desc *desc)
{
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion runs the gather kernels: it needs planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion runs the gather kernels: MVHMR_VARIANT_BRICK is not served");
    return MVHMR_OK;
}
int lens_refused(const mvhmr_unproject_desc *desc, const Call &c)
{
    if (c.view_mask) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion with a view mask is not built yet: un-project the masked samples without a lens");
    if (c.view_weights) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion with view weights is not built yet: un-project the weighted samples without a lens");
    if (c.visible) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion with visibility-aware aggregation is not built yet: the seeing test is pin-hole");
    if (c.view_confidence) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion with view confidence maps is not built yet: un-project those samples without a lens");
    if (c.feature_index) return fail(MVHMR_ERR_UNSUPPORTED, "lens distortion with a feature_index is not built yet: un-project the shared samples without a lens");
    return lens_shape_refused(desc);
}
// ---- cross-view variance (include/mvhmr_unproject.h): the route of the visible calls -- the gather family with the per-tap
// scatter backward and the geometry kernels, which launch their *_moments kernels (Problem::moments); with a mask the views are packed exactly
// as for a masked call, without one nothing is packed or copied.  The variance is taken around the mean: desc->method must say so.
int moments_refused(const mvhmr_unproject_desc *desc, int moments)
{
    if (moments != MVHMR_MOMENTS_VAR && moments != MVHMR_MOMENTS_MEANVAR)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "moments must be MVHMR_MOMENTS_VAR (1) or MVHMR_MOMENTS_MEANVAR (2)");
    if (desc->method != MVHMR_AGG_MEAN)
        return fail(MVHMR_ERR_UNSUPPORTED, "the cross-view variance is taken around the mean: desc->method must be MVHMR_AGG_MEAN (got %d)", desc->method);
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD || desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "the cross-view variance needs planar or channels-last features (quad-planar copies: pass the planar features)");
    if (desc->variant == MVHMR_VARIANT_BRICK)
        return fail(MVHMR_ERR_UNSUPPORTED, "the cross-view variance runs the gather kernels: MVHMR_VARIANT_BRICK is not served");
    return MVHMR_OK;
}
// whether the descriptor can take what the record selects: a shared or a lens call answers for itself, the others for each selection
int call_refused(const mvhmr_unproject_desc *desc, const Call &c)
{
    if (c.family == MVHMR_FAMILY_SHARED) return shared_refused(desc, c);
    if (c.family == MVHMR_FAMILY_LENS) return lens_refused(desc, c);
    int rc = MVHMR_OK;
    if (moments_of(c)) return moments_refused(desc, moments_of(c));      // (the checks of a visible and of a masked call are among its own)
    if (seeing(c) && (rc = visible_refused(desc)) != MVHMR_OK) return rc;
    if (c.view_confidence && (rc = confidence_refused(desc)) != MVHMR_OK) return rc;
    if (c.view_mask && (rc = mask_refused(desc)) != MVHMR_OK) return rc;
    return c.view_weights ? weights_refused(desc) : MVHMR_OK;
}
// the kinds of plan: every view, a mask, weights (with or without a mask), the seeing views of every voxel (with or without a mask),
// confidence maps (with or without a mask, with or without the seeing test); Shared: shared feature maps (no head: nothing is packed);
// Lens: lens distortion (no head either: the plain plan of the gather variant)
// Moments: the cross-view variance (with or without a mask, with or without the seeing test)
enum class Pack { None, Masked, Weighted, Visible, Confidence, Shared, Lens, Moments };
// the plan a call runs on.  A lens call takes the lens plan with or without records; a shared call without an index is the plain call
// with the gather variant forced (index_route)
Pack pack_of(const Call &c)
{
    if (c.family == MVHMR_FAMILY_LENS) return Pack::Lens;
    if (c.family == MVHMR_FAMILY_SHARED) return c.feature_index ? Pack::Shared : Pack::None;
    return moments_of(c) ? Pack::Moments : c.view_confidence ? Pack::Confidence : seeing(c) ? Pack::Visible : c.view_weights ? Pack::Weighted : c.view_mask ? Pack::Masked : Pack::None;
}
// the plan a workspace query sizes: the family's own, which covers every call the family degrades to
Pack pack_of_family(int family)
{
    constexpr Pack kPacks[] = {Pack::None, Pack::Masked, Pack::Weighted, Pack::Visible, Pack::Confidence, Pack::Shared, Pack::Lens, Pack::Moments};
    return kPacks[family];
}
// the plan whose workspace a plan's total also covers: a weighted or visible call's serves the masked one, a masked call's the unmasked one
Pack pack_below(Pack pack) { return pack == Pack::Masked || pack == Pack::Shared ? Pack::None : Pack::Masked; }
// the descriptor and problem of the packed call; view_count is set once the table exists (pack_views)
void mask_route(mvhmr_unproject_desc *desc, Problem *p, Pack pack)
{
    desc->variant = MVHMR_VARIANT_GATHER;
    p->masked = 1;
    p->visible = pack == Pack::Visible || pack == Pack::Moments;   // (a confidence or moments call's flag is set from the call's own: confidence_route, moments_route)
    p->conf = pack == Pack::Confidence;
    p->moments = pack == Pack::Moments ? MVHMR_MOMENTS_MEANVAR : 0;   // (the plans read it as a flag; moments_route sets the call's own)
}
// a moments call composes with the seeing test: both ride in the problem once the plan exists
void moments_route(Problem &p, const Call &c)
{
    if (!moments_of(c)) return;
    p.visible = seeing(c);
    p.moments = moments_of(c);
}
// a confidence call reads the caller's maps (no mask) or the packed ones (pack_views), and composes with the seeing test
void confidence_route(Problem &p, const Call &c)
{
    if (!confidence_of(c)) return;
    p.visible = seeing(c);
    if (!p.confidence) p.confidence = confidence_of(c);
}
// a lens call: the records ride in the problem (null: the plain gather call).  A shared call: the index and the volume count ride in the
// problem (the plans read the count: the geometry partials are per volume); a null index with volumes == batch is the plain call with the
// gather variant (Problem::volumes stays 0)
void index_route(const Call &c, mvhmr_unproject_desc *dq, const mvhmr_unproject_desc **desc, Problem *p)
{
    if (c.family == MVHMR_FAMILY_LENS) p->lens = c.lens;
    if (c.family != MVHMR_FAMILY_SHARED) return;
    if (c.feature_index) {
        p->feature_index = c.feature_index;
        p->volumes = c.volumes;
        return;
    }
    *dq = **desc;
    dq->variant = MVHMR_VARIANT_GATHER;
    *desc = dq;
}
// the plain call with the gather variant: what a null index runs, and a workspace every shared plan's total covers
mvhmr_unproject_desc gather_twin(const mvhmr_unproject_desc *desc)
{
    mvhmr_unproject_desc d = *desc;
    d.variant = MVHMR_VARIANT_GATHER;
    return d;
}
size_t conf_map_bytes(const Problem &p) { return (size_t)p.H * p.W * sizeof(float); }                   // one view's confidence map
size_t masked_view_bytes(const Problem &p) { return (size_t)p.C * p.H * p.W * feat_elem(p); }   // one view, planar or channels-last (C4 == C)

// ---- workspace plans.  One plan per kind of call says which route runs and where every region of the workspace lies; it is computed
// by one function from (descriptor, problem, deterministic, masked).  The *_workspace_bytes queries return its total, the launch
// sequences read its offsets: no other code sizes or places a region.
constexpr size_t kNoRegion = ~(size_t)0;
struct Arena {                                  // regions one behind the other; every size handed in is a multiple of kAlign
    size_t top = 0;
    size_t take(size_t bytes) { const size_t at = top; top += bytes; return at; }
};
unsigned char *at(void *workspace, size_t offset) { return offset == kNoRegion ? nullptr : static_cast<unsigned char *>(workspace) + offset; }

// a masked call's head: table + packed features (+ the packed gradient); the unmasked route's regions lie behind it
struct MaskHead {
    size_t table = kNoRegion, feat = kNoRegion, grad = kNoRegion;
    size_t conf = kNoRegion;                    // a confidence call's maps packed in slot order
};
MaskHead plan_mask_head(Arena &a, const Problem &p, int copies, Pack pack)
{
    MaskHead h;
    h.table = a.take(align_up(pack == Pack::Weighted ? weighted_view_table_bytes(p.B, p.V) : view_table_bytes(p.B, p.V)));
    h.feat = a.take(align_up((size_t)p.B * p.V * masked_view_bytes(p)));
    if (copies > 1) h.grad = a.take(align_up((size_t)p.B * p.V * masked_view_bytes(p)));
    if (pack == Pack::Confidence) h.conf = a.take(align_up((size_t)p.B * p.V * conf_map_bytes(p)));
    return h;
}
// builds the table, packs the features; from here on the call reads the packed features and projections
int pack_views(const MaskHead &h, const Call &c, void *workspace, const void **features, const float **proj, Problem &p, hipStream_t s)
{
    void *table = at(workspace, h.table);
    const float *weights = weights_of(c), *confidence = confidence_of(c);
    int rc = launched(weights ? launch_view_table_weighted(mask_of(c), weights, *proj, table, p.B, p.V, s) : launch_view_table(mask_of(c), *proj, table, p.B, p.V, s),
                      "view table");
    if (rc != MVHMR_OK) return rc;
    if (weights) p.view_weights = view_table_weights(table, p.B, p.V);
    rc = launched(launch_view_pack(*features, at(workspace, h.feat), table, p.B, p.V, masked_view_bytes(p), s), "view pack");
    if (rc != MVHMR_OK) return rc;
    if (confidence) {
        rc = launched(launch_view_pack(confidence, at(workspace, h.conf), table, p.B, p.V, conf_map_bytes(p), s), "confidence pack");
        if (rc != MVHMR_OK) return rc;
        p.confidence = reinterpret_cast<const float *>(at(workspace, h.conf));
    }
    p.view_count = view_table_counts(table);
    *features = at(workspace, h.feat);
    *proj = view_table_proj(table, p.B, p.V);
    return MVHMR_OK;
}

enum class Fwd { Gated, Brick, Gather };        // Gated: both variants are launched, the device-side brick count lets one run
struct ForwardPlan {
    mvhmr_unproject_desc desc;                  // what the kernels run on: the caller's descriptor and problem, or those of the packed call
    Problem p;
    Fwd route;
    MaskHead head;
    size_t staged = kNoRegion;                  // the converted feature copy (gated: either layout); none = the features are read as they are
    size_t gate = kNoRegion;
    size_t total = 0;                           // a masked call's workspace also serves the unmasked one (a null mask)
};
ForwardPlan plan_forward(const mvhmr_unproject_desc *desc, const Problem &p, Pack pack)
{
    ForwardPlan f;
    Arena a;
    f.desc = *desc;
    f.p = p;
    if (pack == Pack::Lens) {
        f.desc.variant = MVHMR_VARIANT_GATHER;
    } else if (pack != Pack::None) {
        mask_route(&f.desc, &f.p, pack);
        if (pack != Pack::Shared) f.head = plan_mask_head(a, p, 1, pack);
    }
    const mvhmr_unproject_desc *d = &f.desc;
    const bool brick = pick_variant(d, f.p) == MVHMR_VARIANT_BRICK;
    f.route = geometry_gated(d, f.p) ? Fwd::Gated : brick ? Fwd::Brick : Fwd::Gather;
    if (d->feat_layout == MVHMR_LAYOUT_BVHWC || d->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E) {
        // read as they are
    } else if (f.route == Fwd::Gated) {
        f.staged = a.take(conv_bytes(f.p));
        f.gate = a.take(kGateBytes);
    } else if (!brick) {
        f.staged = a.take(featT_bytes(f.p));
    } else if (d->feat_layout == MVHMR_LAYOUT_BVCHW) {
        f.staged = a.take(brick_workspace_bytes(f.p));
    }
    // (a weighted call's workspace also serves the masked one, a masked call's the unmasked one)
    if (pack == Pack::Lens) {                                                                                   // (also covers the plain call as the descriptor has it)
        f.total = max_size(a.top, plan_forward(desc, p, Pack::None).total);
        return f;
    }
    f.total = pack == Pack::None ? a.top : max_size(a.top, plan_forward(desc, p, pack_below(pack)).total);
    if (pack == Pack::Confidence || pack == Pack::Moments) f.total = max_size(f.total, plan_forward(desc, p, Pack::Visible).total);      // (a null map is the visible call; a moments query covers its visible twin)
    if (pack == Pack::Shared) {                                                                                 // (a null index is the plain gather call)
        const mvhmr_unproject_desc dg = gather_twin(desc);
        f.total = max_size(f.total, plan_forward(&dg, p, Pack::None).total);
    }
    return f;
}

// The deterministic mode of the feature backward (include/mvhmr_unproject.h) runs the brick kernels' deterministic
// instances where the default's rule takes the bricks (not gated: their slow path serves windows that do not fit, and no host
// synchronisation is needed), the plane kernels where it takes those (no global atomics), else k_bwd_gather_det.  The brick and gather
// routes run the scale pass first and a conversion pass after.
bool det_uses_brick(const mvhmr_unproject_desc *d, const Problem &p) { return bwd_uses_brick(d, p) && brick_bwd_det_supported(p); }
bool det_uses_plane(const mvhmr_unproject_desc *d, const Problem &p) { return !det_uses_brick(d, p) && bwd_uses_plane(d, p); }
size_t det_acc_bytes(const Problem &p) { return align_up((size_t)p.B * p.V * p.H * p.W * p.C4 * sizeof(long long)); }

enum class Bwd { GatedBrickPlane, GatedBrickGather, Brick, Plane, Scatter, DetBrick, DetGather };
struct BackwardPlan {
    mvhmr_unproject_desc desc;                  // as in ForwardPlan
    Problem p;
    Bwd route;
    MaskHead head;
    size_t staged = kNoRegion;                  // the converted feature copy
    size_t acc = kNoRegion;                     // fp32 (default) or int64 (deterministic) accumulator; none = grad_features itself (Scatter)
    size_t table = kNoRegion;                   // the plane kernels' tap table (a gated call: where the brick side's accumulator is)
    size_t scale = kNoRegion;                   // deterministic: the scale pass's output
    size_t gate = kNoRegion;
    size_t total = 0;                           // deterministic: also serves the default route; masked: also the unmasked call
};
// the plane kernels read the quad copy: the caller's own, or one made from planar features
void place_plane_backward(BackwardPlan &b, Arena &a)
{
    b.route = Bwd::Plane;
    if (b.desc.feat_layout == MVHMR_LAYOUT_BVCHW) b.staged = a.take(brick_workspace_bytes(b.p));
    b.table = a.take(align_up(plane_table_bytes(b.p)));
}
void place_default_backward(BackwardPlan &b, Arena &a)
{
    const mvhmr_unproject_desc *d = &b.desc;
    const Problem &p = b.p;
    if (geometry_gated_bwd(d, p) && bwd_uses_brick(d, p)) {
        b.route = bwd_uses_plane(d, p) ? Bwd::GatedBrickPlane : Bwd::GatedBrickGather;
        b.staged = a.take(conv_bytes(p));
        b.acc = b.table = a.take(bwd_mid_bytes(d, p));
        b.gate = a.take(kGateBytes);
    } else if (bwd_uses_brick(d, p)) {
        b.route = Bwd::Brick;
        b.staged = a.take(brick_workspace_bytes(p));        // reserved for quad-planar features too, which are read as they are
        b.acc = a.take(gradT_bytes(p));
    } else if (bwd_uses_plane(d, p)) {
        place_plane_backward(b, a);
    } else {
        b.route = Bwd::Scatter;
        if (d->feat_layout != MVHMR_LAYOUT_BVHWC) b.staged = a.take(featT_bytes(p));
        if (!grad_in_place(d, p)) b.acc = a.take(gradT_bytes(p));
    }
}
void place_det_backward(BackwardPlan &b, Arena &a)
{
    const mvhmr_unproject_desc *d = &b.desc;
    const Problem &p = b.p;
    if (det_uses_plane(d, p)) return place_plane_backward(b, a);        // no global atomics: deterministic as it is
    const bool brick = det_uses_brick(d, p);
    b.route = brick ? Bwd::DetBrick : Bwd::DetGather;
    if (d->feat_layout != (brick ? MVHMR_LAYOUT_QUAD : MVHMR_LAYOUT_BVHWC)) b.staged = a.take(brick ? brick_workspace_bytes(p) : featT_bytes(p));
    b.acc = a.take(det_acc_bytes(p));
    b.scale = a.take(align_up(det_scale_bytes(p)));                      // (every family's: unproject_det.hip has the one layout)
}
BackwardPlan plan_backward(const mvhmr_unproject_desc *desc, const Problem &p, bool det, Pack pack)
{
    BackwardPlan b;
    Arena a;
    b.desc = *desc;
    b.p = p;
    if (pack == Pack::Lens) {
        b.desc.variant = MVHMR_VARIANT_GATHER;
    } else if (pack != Pack::None) {
        mask_route(&b.desc, &b.p, pack);
        if (pack != Pack::Shared) b.head = plan_mask_head(a, p, 2, pack);
    }
    if (det) {
        BackwardPlan dflt = b;
        Arena da = a;
        place_default_backward(dflt, da);
        place_det_backward(b, a);
        a.top = max_size(a.top, da.top);
    } else {
        place_default_backward(b, a);
    }
    if (pack == Pack::Lens) {
        b.total = max_size(a.top, plan_backward(desc, p, det, Pack::None).total);
        return b;
    }
    b.total = pack == Pack::None ? a.top : max_size(a.top, plan_backward(desc, p, det, pack_below(pack)).total);
    if (pack == Pack::Confidence || pack == Pack::Moments) b.total = max_size(b.total, plan_backward(desc, p, det, Pack::Visible).total);
    if (pack == Pack::Shared) {
        const mvhmr_unproject_desc dg = gather_twin(desc);
        b.total = max_size(b.total, plan_backward(&dg, p, det, Pack::None).total);
    }
    return b;
}

// Gradient w.r.t. proj and coords / the pose: the channels-last feature copy k_bwd_geom reads (none for channels-last input), then the
// fp32 partials of grad_proj and (cuboid) of the pose gradients.  desc->variant plays no part.
struct GeometryPlan {
    mvhmr_unproject_desc desc;                  // as in ForwardPlan
    Problem p;
    MaskHead head;
    size_t packed_grad_proj = kNoRegion;        // masked: grad_proj (B,V,3,4) in slot order, unpacked at the end
    size_t staged = kNoRegion;
    size_t part = kNoRegion, pose_part = kNoRegion;
    size_t packed_grad_weights = kNoRegion;     // weighted: grad_weights (B,V) in slot order, unpacked at the end; weight_part: its fp32 partials
    size_t weight_part = kNoRegion;
    // confidence: grad_confidence (B,V,Hf,Wf) in slot order, the (B,V,N) fp32 stream of sum_channels dc, the int64 map and the (B,V) maxima
    size_t packed_grad_conf = kNoRegion, conf_stream = kNoRegion, conf_acc = kNoRegion, conf_max = kNoRegion;
    size_t total = 0;
};
GeometryPlan plan_geometry(const mvhmr_unproject_desc *desc, const Problem &p, bool cuboid, Pack pack)
{
    GeometryPlan g;
    Arena a;
    g.desc = *desc;
    g.p = p;
    if (pack == Pack::Lens) pack = Pack::None;             // (desc->variant plays no part: the plain plan)
    if (pack != Pack::None) {
        mask_route(&g.desc, &g.p, pack);
    }
    if (pack != Pack::None && pack != Pack::Shared) {
        g.head = plan_mask_head(a, p, 1, pack);
        g.packed_grad_proj = a.take(align_up((size_t)p.B * p.V * 12 * sizeof(float)));
    }
    if (pack == Pack::Weighted) {
        g.packed_grad_weights = a.take(align_up((size_t)p.B * p.V * sizeof(float)));
        g.weight_part = a.take(align_up(geom_weight_partial_bytes(p)));
    }
    if (pack == Pack::Confidence) {
        g.packed_grad_conf = a.take(align_up((size_t)p.B * p.V * conf_map_bytes(p)));
        g.conf_stream = a.take(align_up(conf_grad_stream_bytes(p)));
        g.conf_acc = a.take(align_up(conf_grad_acc_bytes(p)));
        g.conf_max = a.take(align_up(conf_grad_max_bytes(p)));
    }
    if (desc->feat_layout != MVHMR_LAYOUT_BVHWC) g.staged = a.take(featT_bytes(p));
    // (shared feature maps: the partials are the only per-volume regions)
    g.part = a.take(align_up(pack == Pack::Shared ? shared_geom_partial_bytes(p) : geom_partial_bytes(p)));
    if (cuboid) g.pose_part = a.take(align_up(pack == Pack::Shared ? shared_pose_partial_bytes(p) : pose_partial_bytes(p)));
    g.total = pack == Pack::None ? a.top : max_size(a.top, plan_geometry(desc, p, cuboid, pack_below(pack)).total);
    if (pack == Pack::Confidence || pack == Pack::Moments) g.total = max_size(g.total, plan_geometry(desc, p, cuboid, Pack::Visible).total);
    return g;
}

// ---- the pieces every route shares
// channels-last copy, in the feature dtype, of whatever layout came in
int stage_channels_last(const mvhmr_unproject_desc *d, const void *features, void *dst, const Problem &p, hipStream_t s)
{
    return launched(d->feat_layout == MVHMR_LAYOUT_QUAD ? launch_quad_to_channels_last(features, dst, p, s) : launch_to_channels_last(features, dst, p, s),
                    "layout pass");
}
int clear_gradient(void *acc, const Problem &p, size_t elem, hipStream_t s)
{
    return launched(hipMemsetAsync(acc, 0, (size_t)p.B * p.V * p.H * p.W * p.C4 * elem, s), "gradient clear");
}
// the forward gate's answer fetched to the host: both mvhmr_unproject_query_variant forms
int query_variant(const mvhmr_unproject_desc *desc, const VolumeSource &v, const float *proj, void *hip_stream)
{
    Problem p;
    if (check_desc(desc, &p) != MVHMR_OK) return -1;
    const int variant = pick_variant(desc, p);
    if (variant_conflict(desc, p, variant) != MVHMR_OK) return -1;
    if (desc->variant != MVHMR_VARIANT_AUTO || !brick_fwd_preferred(p)) return variant;   // nothing to decide
    Coords coords;
    if (!proj || make_coords(v, p, &coords) != MVHMR_OK) { fail(MVHMR_ERR_INVALID_ARGUMENT, v.cuboid ? "null pointer" : "proj / coords must be non-null"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int *count = nullptr, host = 0;
    if (hipMalloc(&count, sizeof(int)) != hipSuccess) { fail(MVHMR_ERR_LAUNCH, "query: allocation failed"); return -1; }
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    const GateGeom g = brick_fwd_gate_geom(p);
    if (e == hipSuccess) e = launch_brick_gate(proj, coords, count, g, p, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&host, count, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(count);
    if (e != hipSuccess) { fail(MVHMR_ERR_LAUNCH, "query: %s", hipGetErrorString(e)); return -1; }
    return host <= brick_count(p, g) / 8 ? MVHMR_VARIANT_BRICK : MVHMR_VARIANT_GATHER;
}

// ---- forward
int run_forward(const mvhmr_unproject_desc *desc, const Call &c, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    Problem p0;
    Coords coords;
    int rc = open_call(desc, placing_of(c), &p0, &coords);
    if (rc != MVHMR_OK) return rc;
    const void *features = c.features;
    const float *proj = c.proj;
    void *out = c.out;
    if (!features || !proj || !out) return fail(MVHMR_ERR_INVALID_ARGUMENT, "features / proj / out must be non-null");
    if ((rc = call_refused(desc, c)) != MVHMR_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    mvhmr_unproject_desc dq;
    index_route(c, &dq, &desc, &p0);
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E) {
        // the quad-planar copy times log2(e): only the wave-specialised softmax forward reads it (mvhmr_preferred_layout says when)
        if (!brick_fwd_prescales(p0) || desc->variant == MVHMR_VARIANT_GATHER)
            return fail(MVHMR_ERR_UNSUPPORTED, "MVHMR_LAYOUT_QUAD_LOG2E feeds the softmax brick forward of 3 / 4 views with an fp32 volume only "
                                               "(ask mvhmr_preferred_layout)");
        dq = *desc;
        dq.feat_layout = MVHMR_LAYOUT_QUAD;
        dq.variant = MVHMR_VARIANT_BRICK;
        desc = &dq;
        p0.feat_log2e = 1;
    }
    ForwardPlan f = plan_forward(desc, p0, pack_of(c));
    desc = &f.desc;
    Problem &p = f.p;
    rc = variant_conflict(desc, p, pick_variant(desc, p));
    if (rc != MVHMR_OK) return rc;
    rc = check_ws(workspace, workspace_bytes, f.total);
    if (rc != MVHMR_OK) return rc;
    if (packed(c) && (rc = pack_views(f.head, c, workspace, &features, &proj, p, s)) != MVHMR_OK) return rc;
    confidence_route(p, c);
    moments_route(p, c);
    // planar input whose staged copy this call makes itself: scaled by log2(e) when the kernel that reads it wants that
    if (desc->feat_layout == MVHMR_LAYOUT_BVCHW && brick_fwd_prescales(p)) p.feat_log2e = 1;

    void *staged = at(workspace, f.staged);
    switch (f.route) {
    case Fwd::Gated: {
        rc = arm_gate(p, at(workspace, f.gate), proj, coords, brick_fwd_gate_geom(p), s);
        if (rc != MVHMR_OK) return rc;
        const bool quad = desc->feat_layout == MVHMR_LAYOUT_QUAD;
        if (!quad) {
            rc = launched(launch_to_quad_planar_t(features, staged, p, s), "layout pass");
            if (rc != MVHMR_OK) return rc;
        }
        rc = stage_channels_last(desc, features, staged, p, s);
        if (rc != MVHMR_OK) return rc;
        rc = launched(launch_fwd_brick(quad ? features : staged, proj, coords, out, p, s), "brick forward");
        if (rc != MVHMR_OK) return rc;
        return launched(launch_fwd_gather(staged, proj, coords, out, p, s), "gather forward");
    }
    case Fwd::Brick:
        if (staged) {
            rc = launched(launch_to_quad_planar_t(features, staged, p, s), "layout pass");
            if (rc != MVHMR_OK) return rc;
        }
        return launched(launch_fwd_brick(staged ? staged : features, proj, coords, out, p, s), "brick forward");
    case Fwd::Gather:
        if (staged) {
            rc = stage_channels_last(desc, features, staged, p, s);
            if (rc != MVHMR_OK) return rc;
        }
        if (p.feature_index) return launched(launch_fwd_gather_shared(staged ? staged : features, proj, coords, out, p, s), "shared gather forward");
        if (p.lens) return launched(launch_fwd_gather_lens(staged ? staged : features, proj, coords, out, p, s), "lens gather forward");
        if (p.moments) return launched(launch_fwd_gather_moments(staged ? staged : features, proj, coords, out, p, s), "moments gather forward");
        return launched(launch_fwd_gather(staged ? staged : features, proj, coords, out, p, s), "gather forward");
    }
    return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown forward route");
}

// ---- feature backward.  The default and the deterministic form share the opening (validation, plan, view packing) and the plane
// route; their launch sequences differ in accumulator type, scale pass and conversion pass and are kept apart.
struct BackwardArgs {
    const void *grad_out, *features;
    const float *proj;
    const Coords *coords;
    void *grad_features, *workspace;
    hipStream_t s;
};

// the quad copy for the plane kernels (planar input), then the kernels: no global atomics, deterministic as they are
int launch_plane_route(const BackwardPlan &b, const BackwardArgs &c)
{
    void *staged = at(c.workspace, b.staged);
    if (staged) {
        const int rc = launched(launch_to_quad_planar_t(c.features, staged, b.p, c.s), "layout pass");
        if (rc != MVHMR_OK) return rc;
    }
    return launched(launch_bwd_plane(staged ? staged : c.features, c.grad_out, c.proj, *c.coords, c.grad_features, at(c.workspace, b.table), b.p, c.s),
                    "plane backward");
}

int launch_backward_default(BackwardPlan &b, const BackwardArgs &c)
{
    const mvhmr_unproject_desc *desc = &b.desc;
    Problem &p = b.p;
    const Coords &coords = *c.coords;
    hipStream_t s = c.s;
    const bool quad = desc->feat_layout == MVHMR_LAYOUT_QUAD;
    void *staged = at(c.workspace, b.staged);
    float *acc = reinterpret_cast<float *>(at(c.workspace, b.acc));
    int rc;
    switch (b.route) {
    case Bwd::GatedBrickPlane:
    case Bwd::GatedBrickGather:
    case Bwd::Brick: {
        // The brick side: the column-major quad copy (the caller's own when the features came quad-planar), LDS windows, float-atomic
        // flush into the quad-planar `acc`, layout pass.  A gated call launches its gather side as well, and the device-side brick
        // count lets one side run: the per-tap scatter on a channels-last copy into a channels-last `acc`, or the plane kernels, which
        // read the quad copy too (so it is made ungated: either side needs it) and have their scratch where `acc` would be.
        const bool scatter_side = b.route == Bwd::GatedBrickGather, plane_side = b.route == Bwd::GatedBrickPlane;
        if (b.route != Bwd::Brick) {
            rc = arm_gate(p, at(c.workspace, b.gate), c.proj, coords, brick_bwd_gate_geom(p), s);
            if (rc != MVHMR_OK) return rc;
        }
        if (!quad) {
            Problem pc = p;
            if (plane_side) pc.gate_count = nullptr;
            rc = launched(launch_to_quad_planar_t(c.features, staged, pc, s, true), "layout pass");
            if (rc != MVHMR_OK) return rc;
        }
        const void *featK = quad ? c.features : staged;
        if (scatter_side) {
            rc = stage_channels_last(desc, c.features, staged, p, s);
            if (rc != MVHMR_OK) return rc;
        }
        rc = clear_gradient(acc, p, sizeof(float), s);
        if (rc != MVHMR_OK) return rc;
        rc = launched(launch_bwd_brick(featK, c.grad_out, c.proj, coords, acc, p, s), "brick backward");
        if (rc != MVHMR_OK) return rc;
        if (scatter_side) {
            rc = launched(launch_bwd_gather(c.grad_out, staged, c.proj, coords, acc, p, s), "gather backward");
            if (rc != MVHMR_OK) return rc;
        }
        rc = launched(launch_quad_grad_to_planar(acc, c.grad_features, p, s), "gradient layout pass");
        if (rc != MVHMR_OK || b.route == Bwd::Brick) return rc;
        if (scatter_side) return launched(launch_grad_to_planar(acc, c.grad_features, p, s), "gradient layout pass");
        return launched(launch_bwd_plane(featK, c.grad_out, c.proj, coords, c.grad_features, at(c.workspace, b.table), p, s), "plane backward");
    }
    case Bwd::Plane:
        return launch_plane_route(b, c);
    case Bwd::Scatter: {
        if (staged) {
            rc = stage_channels_last(desc, c.features, staged, p, s);
            if (rc != MVHMR_OK) return rc;
        }
        float *gradT = acc ? acc : static_cast<float *>(c.grad_features);      // in place: fp32 channels-last grad_features is the accumulator
        rc = clear_gradient(gradT, p, sizeof(float), s);
        if (rc != MVHMR_OK) return rc;
        rc = p.feature_index ? launched(launch_bwd_gather_shared(c.grad_out, staged ? staged : c.features, c.proj, coords, gradT, p, s), "shared gather backward")
             : p.lens        ? launched(launch_bwd_gather_lens(c.grad_out, staged ? staged : c.features, c.proj, coords, gradT, p, s), "lens gather backward")
             : p.moments     ? launched(launch_bwd_gather_moments(c.grad_out, staged ? staged : c.features, c.proj, coords, gradT, p, s), "moments gather backward")
                             : launched(launch_bwd_gather(c.grad_out, staged ? staged : c.features, c.proj, coords, gradT, p, s), "gather backward");
        if (rc != MVHMR_OK || !acc) return rc;
        if (desc->feat_layout != MVHMR_LAYOUT_BVHWC) return launched(launch_grad_to_planar(gradT, c.grad_features, p, s), "gradient layout pass");   // planar gradient for planar and quad-planar features alike
        return launched(launch_grad_cast(gradT, c.grad_features, p, s), "gradient cast");
    }
    default:
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown backward route");
    }
}

int launch_backward_det(const BackwardPlan &b, const BackwardArgs &c)
{
    const mvhmr_unproject_desc *desc = &b.desc;
    const Problem &p = b.p;
    const Coords &coords = *c.coords;
    hipStream_t s = c.s;
    if (b.route == Bwd::Plane) return launch_plane_route(b, c);
    const bool brick = b.route == Bwd::DetBrick;
    if (!brick && desc->feat_layout == MVHMR_LAYOUT_QUAD && !quad_to_channels_last_supported(p))
        return fail(MVHMR_ERR_UNSUPPORTED, "deterministic backward from quad-planar features of this shape: needs C <= 4092 and B * V <= 65535");
    void *staged = at(c.workspace, b.staged);
    int rc;
    if (staged) {
        rc = brick ? launched(launch_to_quad_planar_t(c.features, staged, p, s, true), "layout pass") : stage_channels_last(desc, c.features, staged, p, s);
        if (rc != MVHMR_OK) return rc;
    }
    const void *feat = staged ? staged : c.features;                            // quad-planar (brick) or channels-last (gather) features: as they are
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(at(c.workspace, b.acc));
    void *scale = at(c.workspace, b.scale);
    rc = clear_gradient(acc, p, sizeof(long long), s);
    if (rc != MVHMR_OK) return rc;
    rc = launched(launch_det_scale(c.grad_out, feat, scale, p, s, brick, c.proj, &coords), "deterministic scale pass");
    if (rc != MVHMR_OK) return rc;
    const int *kexp = det_exponents(scale, p);
    if (brick) {
        rc = launched(launch_bwd_brick_det(feat, c.grad_out, c.proj, coords, acc, kexp, p, s), "deterministic brick backward");
        if (rc != MVHMR_OK) return rc;
        return launched(launch_det_quad_to_planar(acc, kexp, c.grad_features, p, s), "gradient layout pass");
    }
    rc = p.feature_index ? launched(launch_bwd_gather_shared_det(c.grad_out, feat, c.proj, coords, acc, kexp, p, s), "deterministic shared gather backward")
         : p.lens        ? launched(launch_bwd_gather_lens_det(c.grad_out, feat, c.proj, coords, acc, kexp, p, s), "deterministic lens gather backward")
         : p.moments     ? launched(launch_bwd_gather_moments_det(c.grad_out, feat, c.proj, coords, acc, kexp, p, s), "deterministic moments gather backward")
                         : launched(launch_bwd_gather_det(c.grad_out, feat, c.proj, coords, acc, kexp, p, s), "deterministic gather backward");
    if (rc != MVHMR_OK) return rc;
    if (desc->feat_layout != MVHMR_LAYOUT_BVHWC) return launched(launch_det_grad_to_planar(acc, kexp, c.grad_features, p, s), "gradient layout pass");
    return launched(launch_det_grad_cast(acc, kexp, c.grad_features, p, s), "gradient cast");
}

int run_backward(const mvhmr_unproject_desc *desc, const Call &c, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    Problem p0;
    Coords coords;
    int rc = open_call(desc, placing_of(c), &p0, &coords);
    if (rc != MVHMR_OK) return rc;
    const void *grad_out = c.grad_out, *features = c.features;
    const float *proj = c.proj;
    void *grad_features = c.grad_features;
    const bool det = c.deterministic != 0;
    if (!grad_out || !features || !proj || !grad_features)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_out / features / proj / grad_features must be non-null");
    if ((rc = call_refused(desc, c)) != MVHMR_OK) return rc;
    mvhmr_unproject_desc dq;
    index_route(c, &dq, &desc, &p0);
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "MVHMR_LAYOUT_QUAD_LOG2E is a forward-only layout: hand the backward the features as they are");
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD && !bwd_uses_brick(desc, p0) && !quad_to_channels_last_supported(p0))
        return fail(MVHMR_ERR_UNSUPPORTED, "backward from quad-planar features of this shape needs the brick backward (fp32, 2 / 4 / 8 views)");
    BackwardPlan b = plan_backward(desc, p0, det, pack_of(c));
    rc = check_ws(workspace, workspace_bytes, b.total);
    if (rc != MVHMR_OK) return rc;
    if (b.desc.variant == MVHMR_VARIANT_BRICK && !bwd_uses_brick(&b.desc, b.p))
        return fail(MVHMR_ERR_UNSUPPORTED, "the brick variant does not support this shape / dtype / layout");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bool slots = packed(c);
    if (slots && (rc = pack_views(b.head, c, workspace, &features, &proj, b.p, s)) != MVHMR_OK) return rc;
    confidence_route(b.p, c);
    moments_route(b.p, c);
    // a masked or weighted call's gradient comes in slot order and is unpacked into view order, absent views zero-filled
    void *grad = slots ? at(workspace, b.head.grad) : grad_features;
    const BackwardArgs args{grad_out, features, proj, &coords, grad, workspace, s};
    rc = det ? launch_backward_det(b, args) : launch_backward_default(b, args);
    if (rc != MVHMR_OK || !slots) return rc;
    return launched(launch_view_unpack(grad, grad_features, at(workspace, b.head.table), b.p.B, b.p.V, masked_view_bytes(b.p), s), "view unpack");
}

// ---- geometry backward
int run_geometry(const mvhmr_unproject_desc *desc, const Call &c, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const VolumeSource v = placing_of(c);
    const void *grad_out = c.grad_out, *features = c.features;
    const float *proj = c.proj;
    float *grad_proj = c.grad_proj, *grad_coords = c.grad_coords, *grad_rot = c.grad_rot, *grad_center = c.grad_center;
    float *grad_weights = c.grad_weights, *grad_confidence = c.grad_confidence;
    const bool mask = packed(c), weighted = weights_of(c), maps = confidence_of(c);
    Problem p0;
    Coords coords;
    int rc = check_desc(desc, &p0);
    if (rc != MVHMR_OK) return rc;
    // (the order and the texts of ABI 4: an unmasked call names the data pointers first, a masked one after the geometry and the outputs)
    const bool data = grad_out && features && proj;
    const char *no_data = "grad_out / features / proj must be non-null", *no_tensor = "grad_out / features / proj / coords must be non-null";
    if (!mask && !data) return fail(MVHMR_ERR_INVALID_ARGUMENT, v.cuboid ? no_data : no_tensor);
    if (!v.cuboid && !v.coords) return fail(MVHMR_ERR_INVALID_ARGUMENT, no_tensor);
    rc = make_coords(v, p0, &coords);
    if (rc != MVHMR_OK) return rc;
    if (grad_weights && !weighted) return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_weights without view_weights: nothing to differentiate");
    if (grad_confidence && !maps) return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_confidence without view_confidence: nothing to differentiate");
    if (!v.cuboid && !grad_proj && !grad_coords && !grad_weights && !grad_confidence)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, weighted ? "grad_proj, grad_coords and grad_weights are all null: nothing to compute"
                                                : maps   ? "grad_proj, grad_coords and grad_confidence are all null: nothing to compute"
                                                         : "grad_proj and grad_coords are both null: nothing to compute");
    if (v.cuboid && !grad_proj && !grad_rot && !grad_center && !grad_weights && !grad_confidence)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, weighted ? "grad_proj, grad_rot, grad_center and grad_weights are all null: nothing to compute"
                                                : maps   ? "grad_proj, grad_rot, grad_center and grad_confidence are all null: nothing to compute"
                                                         : "grad_proj, grad_rot and grad_center are all null: nothing to compute");
    if (!data) return fail(MVHMR_ERR_INVALID_ARGUMENT, no_data);
    if ((rc = call_refused(desc, c)) != MVHMR_OK) return rc;
    mvhmr_unproject_desc dq;
    index_route(c, &dq, &desc, &p0);
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E)
        return fail(MVHMR_ERR_UNSUPPORTED, "MVHMR_LAYOUT_QUAD_LOG2E is a forward-only layout: hand the backward the features as they are");
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD && !quad_to_channels_last_supported(p0))
        return fail(MVHMR_ERR_UNSUPPORTED, "quad-planar features of this shape cannot be converted to channels-last (C %% 4 == 0, C <= 4092, B * V <= 65535)");
    GeometryPlan g = plan_geometry(desc, p0, v.cuboid, pack_of(c));
    rc = check_ws(workspace, workspace_bytes, g.total);
    if (rc != MVHMR_OK) return rc;
    const Problem &p = g.p;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (mask && (rc = pack_views(g.head, c, workspace, &features, &proj, g.p, s)) != MVHMR_OK) return rc;
    confidence_route(g.p, c);
    moments_route(g.p, c);
    // grad_confidence: the kernel's stream of sum_channels dc, then launch_conf_grad (slot order behind the head with a mask, unpacked at the end)
    float *gc = mask && grad_confidence ? reinterpret_cast<float *>(at(workspace, g.packed_grad_conf)) : grad_confidence;
    if (grad_confidence) g.p.conf_stream = reinterpret_cast<float *>(at(workspace, g.conf_stream));
    // a masked call's grad_proj comes in slot order behind the head and is unpacked; the other gradients are per sample
    float *gp = mask && grad_proj ? reinterpret_cast<float *>(at(workspace, g.packed_grad_proj)) : grad_proj;
    void *staged = at(workspace, g.staged);
    if (staged) {
        rc = stage_channels_last(&g.desc, features, staged, p, s);
        if (rc != MVHMR_OK) return rc;
    }
    const void *featT = staged ? staged : features;
    float *part = gp ? reinterpret_cast<float *>(at(workspace, g.part)) : nullptr;
    // grad_weights likewise: fp32 partials, summed into slot order, unpacked (absent views zero-filled)
    float *gw = grad_weights ? reinterpret_cast<float *>(at(workspace, g.packed_grad_weights)) : nullptr;
    float *wpart = grad_weights ? reinterpret_cast<float *>(at(workspace, g.weight_part)) : nullptr;
    if (p.feature_index) {
        // shared feature maps: grad_coords / grad_rot / grad_center are per volume, grad_proj is summed over the volumes that name each sample
        float *pose_part = (grad_rot || grad_center) ? reinterpret_cast<float *>(at(workspace, g.pose_part)) : nullptr;
        return v.cuboid ? launched(launch_bwd_geom_cuboid_shared(grad_out, featT, proj, coords, part, gp, pose_part, grad_rot, grad_center, p, s), "shared cuboid geometry backward")
                        : launched(launch_bwd_geom_shared(grad_out, featT, proj, coords, part, gp, grad_coords, p, s), "shared geometry backward");
    }
    if (v.cuboid) {
        float *pose_part = (grad_rot || grad_center) ? reinterpret_cast<float *>(at(workspace, g.pose_part)) : nullptr;
        rc = launched(launch_bwd_geom_cuboid(grad_out, featT, proj, coords, part, gp, pose_part, grad_rot, grad_center, p, s, wpart, gw), "cuboid geometry backward");
    } else {
        rc = launched(launch_bwd_geom(grad_out, featT, proj, coords, part, gp, grad_coords, p, s, wpart, gw), "geometry backward");
    }
    if (rc == MVHMR_OK && grad_confidence)
        rc = launched(launch_conf_grad(p.conf_stream, proj, coords, reinterpret_cast<unsigned long long *>(at(workspace, g.conf_acc)),
                                       reinterpret_cast<unsigned *>(at(workspace, g.conf_max)), gc, p, s), "confidence gradient");
    if (rc != MVHMR_OK || !mask) return rc;
    if (grad_confidence && (rc = launched(launch_view_unpack(gc, grad_confidence, at(workspace, g.head.table), p.B, p.V, conf_map_bytes(p), s), "view unpack")) != MVHMR_OK)
        return rc;
    if (grad_proj && (rc = launched(launch_view_unpack(gp, grad_proj, at(workspace, g.head.table), p.B, p.V, 12 * sizeof(float), s), "view unpack")) != MVHMR_OK)
        return rc;
    if (!grad_weights) return rc;
    return launched(launch_view_unpack(gw, grad_weights, at(workspace, g.head.table), p.B, p.V, sizeof(float), s), "view unpack");
}

// ---- the visibility bits themselves: no features, no workspace, one kernel
int run_visibility(const mvhmr_unproject_desc *desc, const VolumeSource &v, const float *proj, const uint8_t *view_mask, int32_t *bits, void *hip_stream)
{
    Problem p;
    Coords coords;
    int rc = open_call(desc, v, &p, &coords);
    if (rc != MVHMR_OK) return rc;
    if (!proj || !bits) return fail(MVHMR_ERR_INVALID_ARGUMENT, "proj / bits must be non-null");
    if ((rc = visible_refused(desc)) != MVHMR_OK) return rc;
    return launched(launch_view_visibility(proj, coords, view_mask, bits, p, static_cast<hipStream_t>(hip_stream)), "view visibility");
}

// the workspace queries: a descriptor the call would refuse outright needs none
bool pack_refused(const mvhmr_unproject_desc *desc, Pack pack)
{
    return (pack == Pack::Masked && mask_refused(desc) != MVHMR_OK) || (pack == Pack::Weighted && weights_refused(desc) != MVHMR_OK) ||
           (pack == Pack::Visible && visible_refused(desc) != MVHMR_OK) || (pack == Pack::Confidence && confidence_refused(desc) != MVHMR_OK) ||
           (pack == Pack::Moments && moments_refused(desc, MVHMR_MOMENTS_MEANVAR) != MVHMR_OK);
}
// Only the descriptor and the record's family, placing, volumes and deterministic are read, never a device pointer: what a family degrades
// to with a null pointer is not known here, and its plan's total covers it.
size_t call_need(const mvhmr_unproject_desc *desc, const Call &c, int kind)
{
    Problem p;
    if (check_desc(desc, &p) != MVHMR_OK) return 0;
    const Pack pack = pack_of_family(c.family);
    if (pack == Pack::Shared) {
        if (shared_shape_refused(desc, c.volumes) != MVHMR_OK) return 0;
        p.volumes = c.volumes;
    } else if (pack == Pack::Lens) {
        if (lens_shape_refused(desc) != MVHMR_OK) return 0;
    } else if ((kind != MVHMR_CALL_FORWARD && desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E) || pack_refused(desc, pack)) {
        return 0;
    }
    switch (kind) {
    case MVHMR_CALL_FORWARD: return plan_forward(desc, p, pack).total;
    case MVHMR_CALL_BACKWARD: return plan_backward(desc, p, c.deterministic != 0, pack).total;
    case MVHMR_CALL_GEOMETRY: return plan_geometry(desc, p, c.placing == MVHMR_PLACING_CUBOID, pack).total;
    }
    fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown call kind %d", kind);
    return 0;
}

// where the deterministic backward of this call keeps K (mvhmr_internal_det_exponent_table): run_backward's checks and plan, no launch
int det_exponent_table(const mvhmr_unproject_desc *desc, const Call &c, size_t *offset, size_t *count)
{
    Problem p0;
    int rc = check_desc(desc, &p0);
    if (rc != MVHMR_OK) return rc;
    if (!offset || !count) return fail(MVHMR_ERR_INVALID_ARGUMENT, "offset / count must be non-null");
    if (!c.deterministic) return fail(MVHMR_ERR_INVALID_ARGUMENT, "the exponent table belongs to the deterministic backward: set call->deterministic");
    if ((rc = call_refused(desc, c)) != MVHMR_OK) return rc;
    mvhmr_unproject_desc dq;
    index_route(c, &dq, &desc, &p0);
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E) return fail(MVHMR_ERR_UNSUPPORTED, "MVHMR_LAYOUT_QUAD_LOG2E is a forward-only layout");
    const BackwardPlan b = plan_backward(desc, p0, true, pack_of(c));
    if (b.route == Bwd::Plane) return fail(MVHMR_ERR_UNSUPPORTED, "this call takes the plane backward: no scale pass");
    const unsigned char *base = reinterpret_cast<const unsigned char *>(kAlign);                       // (never read: det_exponents only places K)
    *offset = b.scale + (size_t)(reinterpret_cast<const unsigned char *>(det_exponents(base, b.p)) - base);
    *count = (size_t)b.p.B * b.p.C;
    return MVHMR_OK;
}

// a zeroed record of one family: what every named entry point starts from
Call record(int family, bool deterministic = false)
{
    Call r{};
    r.struct_size = sizeof(Call);
    r.family = family;
    r.deterministic = deterministic;
    return r;
}

}  // namespace

extern "C" {

int mvhmr_abi_version(void) { return MVHMR_ABI_VERSION; }

unsigned long long mvhmr_internal_lds_cache_key(int device, const void *kernel) { return dynamic_lds_cache_key(device, kernel); }

int mvhmr_internal_det_exponent_table(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, size_t *offset, size_t *count)
{
    const int rc = check_call(call);
    return rc != MVHMR_OK ? rc : det_exponent_table(desc, *call, offset, count);
}

const char *mvhmr_last_error(void) { return g_err; }

const char *mvhmr_status_string(int status)
{
    switch (status) {
    case MVHMR_OK: return "ok";
    case MVHMR_ERR_INVALID_ARGUMENT: return "invalid argument";
    case MVHMR_ERR_UNSUPPORTED: return "unsupported";
    case MVHMR_ERR_WORKSPACE: return "workspace";
    case MVHMR_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown status";
    }
}

int mvhmr_unproject_selected_variant(const mvhmr_unproject_desc *desc)
{
    Problem p;
    if (check_desc(desc, &p) != MVHMR_OK) return -1;
    const int variant = pick_variant(desc, p);
    return variant_conflict(desc, p, variant) == MVHMR_OK ? variant : -1;
}

int mvhmr_unproject_query_variant(const mvhmr_unproject_desc *desc, const float *proj, const float *coords, void *hip_stream)
{
    return query_variant(desc, tensor_volume(coords), proj, hip_stream);
}

int mvhmr_unproject_query_variant_cuboid(const mvhmr_unproject_desc *desc, const float *proj, const float *rot, const float *center,
                                         const double position[3], const double sides[3], void *hip_stream)
{
    return query_variant(desc, cuboid_volume(rot, center, position, sides), proj, hip_stream);
}

const char *mvhmr_unproject_forward_kernel_name(const mvhmr_unproject_desc *desc)
{
    Problem p;
    if (check_desc(desc, &p) != MVHMR_OK) return nullptr;
    const int variant = pick_variant(desc, p);
    if (variant_conflict(desc, p, variant) != MVHMR_OK) return nullptr;
    if (variant != MVHMR_VARIANT_BRICK) return "k_fwd_gather";
    if (brick_fwd_ws_shape(p)) return "k_fwd_ws";
    return p.V > 4 ? "k_fwd_brick_groups" : "k_fwd_brick";
}

int mvhmr_unproject_backward_supported(const mvhmr_unproject_desc *desc)
{
    Problem p;
    if (check_desc(desc, &p) != MVHMR_OK) return 0;
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD_LOG2E) return 0;                  // a forward-only layout
    if (desc->variant == MVHMR_VARIANT_BRICK && !bwd_uses_brick(desc, p)) return 0;
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD && !bwd_uses_brick(desc, p) && !quad_to_channels_last_supported(p)) return 0;
    if (desc->feat_layout == MVHMR_LAYOUT_QUAD && desc->variant == MVHMR_VARIANT_GATHER && !quad_to_channels_last_supported(p)) return 0;
    return 1;
}


// ---- the call record: the four functions every un-projection entry point goes through
size_t mvhmr_unproject_call_workspace_bytes(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, int kind)
{
    return check_record(call) == MVHMR_OK ? call_need(desc, *call, kind) : 0;
}

int mvhmr_unproject_forward_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const int rc = check_call(call);
    return rc != MVHMR_OK ? rc : run_forward(desc, *call, workspace, workspace_bytes, hip_stream);
}

int mvhmr_unproject_backward_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const int rc = check_call(call);
    return rc != MVHMR_OK ? rc : run_backward(desc, *call, workspace, workspace_bytes, hip_stream);
}

int mvhmr_unproject_backward_geometry_call(const mvhmr_unproject_desc *desc, const mvhmr_unproject_call *call, void *workspace, size_t workspace_bytes,
                                           void *hip_stream)
{
    const int rc = check_call(call);
    return rc != MVHMR_OK ? rc : run_geometry(desc, *call, workspace, workspace_bytes, hip_stream);
}

// ---- the named entry points (ABI 4): each fills a record from its arguments and calls the record function of its kind.  A name is
// mvhmr_unproject_<kind>[_cuboid][_deterministic][_<family>]; MVHMR_SHIMS writes the four launching names and the four queries of one
// (family, placing) from three tables: what places the volume (PLACE_*, GEOM_*), and per family its arguments behind the placing (ARGS_*),
// the geometry call's own output (GOUT_*) and the query's argument (QARG_*), each with the statements that put them into the record r.
#define PLACE_ARGS_TENSOR const float *coords
#define PLACE_SET_TENSOR r.placing = MVHMR_PLACING_TENSOR, r.coords = coords
#define GEOM_ARGS_TENSOR float *grad_proj, float *grad_coords
#define GEOM_SET_TENSOR r.grad_proj = grad_proj, r.grad_coords = grad_coords
#define PLACE_ARGS_CUBOID const float *rot, const float *center, const double position[3], const double sides[3]
#define PLACE_SET_CUBOID r.placing = MVHMR_PLACING_CUBOID, r.rot = rot, r.center = center, r.position = position, r.sides = sides
#define GEOM_ARGS_CUBOID float *grad_proj, float *grad_rot, float *grad_center
#define GEOM_SET_CUBOID r.grad_proj = grad_proj, r.grad_rot = grad_rot, r.grad_center = grad_center

#define ARGS_PLAIN
#define SET_PLAIN (void)0
#define ARGS_MASKED const uint8_t *view_mask,
#define SET_MASKED r.view_mask = view_mask
#define ARGS_WEIGHTED const uint8_t *view_mask, const float *view_weights,
#define SET_WEIGHTED r.view_mask = view_mask, r.view_weights = view_weights
#define ARGS_VISIBLE const uint8_t *view_mask,
#define SET_VISIBLE r.view_mask = view_mask
#define ARGS_CONFIDENCE const uint8_t *view_mask, const float *view_confidence, int visible,
#define SET_CONFIDENCE r.view_mask = view_mask, r.view_confidence = view_confidence, r.visible = visible != 0
#define ARGS_MOMENTS const uint8_t *view_mask, int32_t visible, int32_t moments,
#define SET_MOMENTS r.view_mask = view_mask, r.visible = visible != 0, r.moments = moments
#define ARGS_SHARED int32_t volumes, const int32_t *feature_index, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible,
#define SET_SHARED r.volumes = volumes, r.feature_index = feature_index, r.view_mask = view_mask, r.view_weights = view_weights, r.view_confidence = view_confidence, r.visible = visible != 0
#define ARGS_LENS const float *lens, const uint8_t *view_mask, const float *view_weights, const float *view_confidence, int visible, const int32_t *feature_index,
#define SET_LENS r.lens = lens, r.view_mask = view_mask, r.view_weights = view_weights, r.view_confidence = view_confidence, r.visible = visible != 0, r.feature_index = feature_index

#define GOUT_PLAIN
#define GOUT_MASKED
#define GOUT_VISIBLE
#define GOUT_MOMENTS
#define GOUT_SHARED
#define GOUT_LENS
#define GOUT_WEIGHTED float *grad_weights,
#define GOUT_CONFIDENCE float *grad_confidence,
#define GSET_PLAIN (void)0
#define GSET_MASKED (void)0
#define GSET_VISIBLE (void)0
#define GSET_MOMENTS (void)0
#define GSET_SHARED (void)0
#define GSET_LENS (void)0
#define GSET_WEIGHTED r.grad_weights = grad_weights
#define GSET_CONFIDENCE r.grad_confidence = grad_confidence

#define QARG_MASKED
#define QARG_WEIGHTED
#define QARG_VISIBLE
#define QARG_CONFIDENCE
#define QARG_MOMENTS
#define QARG_LENS
#define QARG_SHARED , int32_t volumes
#define QSET_MASKED (void)0
#define QSET_WEIGHTED (void)0
#define QSET_VISIBLE (void)0
#define QSET_CONFIDENCE (void)0
#define QSET_MOMENTS (void)0
#define QSET_LENS (void)0
#define QSET_SHARED r.volumes = volumes

#define MVHMR_TAIL void *workspace, size_t workspace_bytes, void *hip_stream
#define MVHMR_LAUNCHERS(F, SFX, P, CUB)                                                                                                                  \
    int mvhmr_unproject_forward##CUB##SFX(const mvhmr_unproject_desc *desc, const void *features, const float *proj, PLACE_ARGS_##P, ARGS_##F void *out,  \
                                          MVHMR_TAIL)                                                                                                    \
    {                                                                                                                                                    \
        Call r = record(MVHMR_FAMILY_##F);                                                                                                               \
        PLACE_SET_##P, SET_##F, r.features = features, r.proj = proj, r.out = out;                                                                       \
        return mvhmr_unproject_forward_call(desc, &r, workspace, workspace_bytes, hip_stream);                                                           \
    }                                                                                                                                                    \
    int mvhmr_unproject_backward##CUB##SFX(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,               \
                                           PLACE_ARGS_##P, ARGS_##F void *grad_features, MVHMR_TAIL)                                                     \
    {                                                                                                                                                    \
        Call r = record(MVHMR_FAMILY_##F);                                                                                                               \
        PLACE_SET_##P, SET_##F, r.grad_out = grad_out, r.features = features, r.proj = proj, r.grad_features = grad_features;                            \
        return mvhmr_unproject_backward_call(desc, &r, workspace, workspace_bytes, hip_stream);                                                          \
    }                                                                                                                                                    \
    int mvhmr_unproject_backward##CUB##_deterministic##SFX(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features,                  \
                                                           const float *proj, PLACE_ARGS_##P, ARGS_##F void *grad_features, MVHMR_TAIL)                  \
    {                                                                                                                                                    \
        Call r = record(MVHMR_FAMILY_##F, true);                                                                                                         \
        PLACE_SET_##P, SET_##F, r.grad_out = grad_out, r.features = features, r.proj = proj, r.grad_features = grad_features;                            \
        return mvhmr_unproject_backward_call(desc, &r, workspace, workspace_bytes, hip_stream);                                                          \
    }                                                                                                                                                    \
    int mvhmr_unproject_backward_geometry##CUB##SFX(const mvhmr_unproject_desc *desc, const void *grad_out, const void *features, const float *proj,      \
                                                    PLACE_ARGS_##P, ARGS_##F GEOM_ARGS_##P, GOUT_##F MVHMR_TAIL)                                         \
    {                                                                                                                                                    \
        Call r = record(MVHMR_FAMILY_##F);                                                                                                               \
        PLACE_SET_##P, SET_##F, GEOM_SET_##P, GSET_##F, r.grad_out = grad_out, r.features = features, r.proj = proj;                                     \
        return mvhmr_unproject_backward_geometry_call(desc, &r, workspace, workspace_bytes, hip_stream);                                                 \
    }
#define MVHMR_QUERY(NAME, F, P, KIND, DET)                                                                                                               \
    size_t NAME##_workspace_bytes(const mvhmr_unproject_desc *desc QARG_##F)                                                                             \
    {                                                                                                                                                    \
        Call r = record(MVHMR_FAMILY_##F, DET);                                                                                                          \
        r.placing = MVHMR_PLACING_##P, QSET_##F;                                                                                                         \
        return mvhmr_unproject_call_workspace_bytes(desc, &r, KIND);                                                                                     \
    }
#define MVHMR_SHIMS(F, SFX, P, CUB)                                                                                                                      \
    MVHMR_LAUNCHERS(F, SFX, P, CUB)                                                                                                                      \
    MVHMR_QUERY(mvhmr_unproject_forward##CUB##SFX, F, P, MVHMR_CALL_FORWARD, false)                                                                      \
    MVHMR_QUERY(mvhmr_unproject_backward##CUB##SFX, F, P, MVHMR_CALL_BACKWARD, false)                                                                    \
    MVHMR_QUERY(mvhmr_unproject_backward##CUB##_deterministic##SFX, F, P, MVHMR_CALL_BACKWARD, true)                                                     \
    MVHMR_QUERY(mvhmr_unproject_backward_geometry##CUB##SFX, F, P, MVHMR_CALL_GEOMETRY, false)
#define MVHMR_FAMILY_SHIMS(F, SFX) MVHMR_SHIMS(F, SFX, TENSOR, ) MVHMR_SHIMS(F, SFX, CUBOID, _cuboid)

// the plain family has no suffix, and the five queries ABI 4 gave it (the forward and feature-backward ones serve both placings)
#define QARG_PLAIN
#define QSET_PLAIN (void)0
MVHMR_LAUNCHERS(PLAIN, , TENSOR, )
MVHMR_LAUNCHERS(PLAIN, , CUBOID, _cuboid)
MVHMR_QUERY(mvhmr_unproject_forward, PLAIN, TENSOR, MVHMR_CALL_FORWARD, false)
MVHMR_QUERY(mvhmr_unproject_backward, PLAIN, TENSOR, MVHMR_CALL_BACKWARD, false)
MVHMR_QUERY(mvhmr_unproject_backward_deterministic, PLAIN, TENSOR, MVHMR_CALL_BACKWARD, true)
MVHMR_QUERY(mvhmr_unproject_backward_geometry, PLAIN, TENSOR, MVHMR_CALL_GEOMETRY, false)
MVHMR_QUERY(mvhmr_unproject_backward_geometry_cuboid, PLAIN, CUBOID, MVHMR_CALL_GEOMETRY, false)
MVHMR_FAMILY_SHIMS(MASKED, _masked)
MVHMR_FAMILY_SHIMS(WEIGHTED, _weighted)
MVHMR_FAMILY_SHIMS(VISIBLE, _visible)
MVHMR_FAMILY_SHIMS(CONFIDENCE, _confidence)
MVHMR_FAMILY_SHIMS(SHARED, _shared)
MVHMR_FAMILY_SHIMS(LENS, _lens)
MVHMR_FAMILY_SHIMS(MOMENTS, _moments)

int mvhmr_unproject_visibility(const mvhmr_unproject_desc *desc, const float *proj, const float *coords, const uint8_t *view_mask, int32_t *bits,
                               void *hip_stream)
{
    return run_visibility(desc, tensor_volume(coords), proj, view_mask, bits, hip_stream);
}

int mvhmr_unproject_visibility_cuboid(const mvhmr_unproject_desc *desc, const float *proj, const float *rot, const float *center,
                                      const double position[3], const double sides[3], const uint8_t *view_mask, int32_t *bits, void *hip_stream)
{
    return run_visibility(desc, cuboid_volume(rot, center, position, sides), proj, view_mask, bits, hip_stream);
}

int mvhmr_preferred_layout(const mvhmr_unproject_desc *desc)
{
    Problem p;
    if (!desc) return -1;
    mvhmr_unproject_desc d = *desc;
    d.feat_layout = MVHMR_LAYOUT_BVCHW;
    if (check_desc(&d, &p) != MVHMR_OK) return -1;
    const int variant = pick_variant(&d, p);
    if (variant_conflict(&d, p, variant) != MVHMR_OK) return -1;
    if (variant != MVHMR_VARIANT_BRICK) return MVHMR_LAYOUT_BVHWC;
    return brick_fwd_prescales(p) ? MVHMR_LAYOUT_QUAD_LOG2E : MVHMR_LAYOUT_QUAD;
}

size_t mvhmr_feature_layout_bytes(const mvhmr_unproject_desc *desc, int dst_layout)
{
    Problem p;
    if (!desc) return 0;
    mvhmr_unproject_desc d = *desc;
    d.feat_layout = MVHMR_LAYOUT_BVCHW;
    if (check_desc(&d, &p) != MVHMR_OK) return 0;
    if (dst_layout == MVHMR_LAYOUT_BVHWC) return featT_bytes(p);
    if (dst_layout == MVHMR_LAYOUT_QUAD || dst_layout == MVHMR_LAYOUT_QUAD_LOG2E) return brick_workspace_bytes(p);   // always fp32, whatever the storage type; (C + 3) / 4 quads per view
    return 0;
}

int mvhmr_convert_features(const mvhmr_unproject_desc *desc, const void *features, int dst_layout, void *dst, void *hip_stream)
{
    Problem p;
    if (!desc) return fail(MVHMR_ERR_INVALID_ARGUMENT, "descriptor is null");
    mvhmr_unproject_desc d = *desc;
    const bool from_channels_last = desc->feat_layout == MVHMR_LAYOUT_BVHWC;      // r04: a channels-last source (to MVHMR_LAYOUT_QUAD only)
    d.feat_layout = MVHMR_LAYOUT_BVCHW;
    int rc = check_desc(&d, &p);
    if (rc != MVHMR_OK) return rc;
    if (!features || !dst) return fail(MVHMR_ERR_INVALID_ARGUMENT, "features / dst must be non-null");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (from_channels_last) {
        if (dst_layout != MVHMR_LAYOUT_QUAD) return fail(MVHMR_ERR_UNSUPPORTED, "channels-last features convert to MVHMR_LAYOUT_QUAD only");
        p.gate_count = nullptr;
        return launched(launch_channels_last_to_quad_planar_t(features, dst, p, s), "layout pass");
    }
    if (dst_layout == MVHMR_LAYOUT_BVHWC) return launched(launch_to_channels_last(features, dst, p, s), "layout pass");
    if (dst_layout == MVHMR_LAYOUT_QUAD) return launched(launch_to_quad_planar_t(features, dst, p, s), "layout pass");
    if (dst_layout == MVHMR_LAYOUT_QUAD_LOG2E) {
        p.feat_log2e = 1;
        return launched(launch_to_quad_planar_t(features, dst, p, s), "layout pass");
    }
    return fail(MVHMR_ERR_INVALID_ARGUMENT, "unknown destination layout %d", dst_layout);
}

// the 1x1-conv GEMMs read their operands (and write the quad-planar copy) with 16-byte accesses
static bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }      // (null, an absent bias, counts as aligned)
static int conv1x1_too_many_maps(int32_t n_maps)
{
    return fail(MVHMR_ERR_UNSUPPORTED, "1x1 conv takes at most %d maps per call (got %d): split the batch", kConv1x1MaxMaps, n_maps);
}

int mvhmr_conv1x1_to_quad(const float *x, const float *weight, const float *bias, void *dst, int32_t n_maps, int32_t c_in, int32_t c_out,
                          int32_t feat_h, int32_t feat_w, void *hip_stream)
{
    if (!x || !weight || !dst) return fail(MVHMR_ERR_INVALID_ARGUMENT, "x / weight / dst must be non-null");
    if (n_maps < 1 || c_in < 1 || c_out < 1 || feat_h < 1 || feat_w < 1) return fail(MVHMR_ERR_INVALID_ARGUMENT, "every dimension must be >= 1");
    if (!aligned16(x) || !aligned16(weight) || !aligned16(bias) || !aligned16(dst))
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "x / weight / bias / dst must be 16-byte aligned");
    if (!conv1x1_quad_supported(c_in, c_out, feat_h, feat_w))
        return fail(MVHMR_ERR_UNSUPPORTED, "fused 1x1 conv needs C_in %% 16 == 0, C_out %% 128 == 0, Hf %% 4 == 0, Wf %% 32 == 0 (got %d -> %d, %dx%d)",
                    c_in, c_out, feat_h, feat_w);
    if (n_maps > kConv1x1MaxMaps) return conv1x1_too_many_maps(n_maps);
    return launched(launch_conv1x1_quad(x, weight, bias, dst, n_maps, c_in, c_out, feat_h, feat_w, static_cast<hipStream_t>(hip_stream)),
                    "fused 1x1 conv");
}

int mvhmr_conv1x1_to_quad_supported(int32_t c_in, int32_t c_out, int32_t feat_h, int32_t feat_w)
{
    return conv1x1_quad_supported(c_in, c_out, feat_h, feat_w) ? 1 : 0;
}

int mvhmr_conv1x1_planar(const float *x, const float *weight, const float *bias, float *dst, int32_t n_maps, int32_t c_in, int32_t c_out,
                         int32_t pixels, void *hip_stream)
{
    if (!x || !weight || !dst) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (n_maps <= 0 || c_in <= 0 || c_out <= 0 || pixels <= 0) return fail(MVHMR_ERR_INVALID_ARGUMENT, "non-positive extent");
    if (!aligned16(x) || !aligned16(weight) || !aligned16(bias) || !aligned16(dst))
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "x / weight / bias / dst must be 16-byte aligned");
    if (!conv1x1_planar_supported(c_in, c_out, pixels))
        return fail(MVHMR_ERR_UNSUPPORTED, "planar 1x1 conv needs C_in %% 16 == 0, C_out %% 128 == 0, pixels %% 128 == 0 (got %d -> %d, %d)", c_in, c_out, pixels);
    if (n_maps > kConv1x1MaxMaps) return conv1x1_too_many_maps(n_maps);
    return launched(launch_conv1x1_planar(x, weight, bias, dst, n_maps, c_in, c_out, pixels, static_cast<hipStream_t>(hip_stream)), "planar 1x1 conv");
}

int mvhmr_conv1x1_planar_supported(int32_t c_in, int32_t c_out, int32_t pixels)
{
    return conv1x1_planar_supported(c_in, c_out, pixels) ? 1 : 0;
}

int mvhmr_conv1x1_wgrad(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int32_t n_maps, int32_t c_in,
                        int32_t c_out, int32_t pixels, void *hip_stream)
{
    if (!grad_y || !x || !grad_weight) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (n_maps <= 0 || c_in <= 0 || c_out <= 0 || pixels <= 0) return fail(MVHMR_ERR_INVALID_ARGUMENT, "non-positive extent");
    if (!aligned16(grad_y) || !aligned16(x)) return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_y / x must be 16-byte aligned");
    if (!conv1x1_wgrad_supported(c_in, c_out, pixels))
        return fail(MVHMR_ERR_UNSUPPORTED, "1x1 conv weight gradient needs C_in %% 128 == 0, C_out %% 128 == 0, pixels %% 32 == 0 (got %d -> %d, %d)", c_in, c_out, pixels);
    return launched(launch_conv1x1_wgrad(grad_y, x, grad_weight, grad_bias, n_maps, c_in, c_out, pixels, static_cast<hipStream_t>(hip_stream)),
                    "1x1 conv weight gradient");
}

int mvhmr_conv1x1_wgrad_supported(int32_t c_in, int32_t c_out, int32_t pixels)
{
    return conv1x1_wgrad_supported(c_in, c_out, pixels) ? 1 : 0;
}

size_t mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(int32_t n_maps, int32_t c_in, int32_t c_out, int32_t pixels)
{
    return conv1x1_wgrad_det_workspace_bytes(n_maps, c_in, c_out, pixels);
}

int mvhmr_conv1x1_wgrad_deterministic(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int32_t n_maps, int32_t c_in,
                                      int32_t c_out, int32_t pixels, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!grad_y || !x || !grad_weight) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (n_maps <= 0 || c_in <= 0 || c_out <= 0 || pixels <= 0) return fail(MVHMR_ERR_INVALID_ARGUMENT, "non-positive extent");
    if (!aligned16(grad_y) || !aligned16(x)) return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_y / x must be 16-byte aligned");
    if (!conv1x1_wgrad_supported(c_in, c_out, pixels))
        return fail(MVHMR_ERR_UNSUPPORTED, "1x1 conv weight gradient needs C_in %% 128 == 0, C_out %% 128 == 0, pixels %% 32 == 0 (got %d -> %d, %d)", c_in, c_out, pixels);
    const int rc = check_ws(workspace, workspace_bytes, conv1x1_wgrad_det_workspace_bytes(n_maps, c_in, c_out, pixels));
    if (rc != MVHMR_OK) return rc;
    return launched(launch_conv1x1_wgrad_det(grad_y, x, grad_weight, grad_bias, workspace, n_maps, c_in, c_out, pixels, static_cast<hipStream_t>(hip_stream)),
                    "deterministic 1x1 conv weight gradient");
}

int mvhmr_triangulate_dlt(const float *proj, const float *points, float *out, int32_t batch, int32_t views, int32_t points_per_sample,
                          void *hip_stream)
{
    if (!proj || !points || !out) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (batch < 1 || views < 2) return fail(MVHMR_ERR_INVALID_ARGUMENT, "batch must be >= 1 and views >= 2 (got %d, %d)", batch, views);
    return launched(launch_triangulate_dlt(proj, points, nullptr, out, batch, views, points_per_sample ? 1 : 0, 0, static_cast<hipStream_t>(hip_stream)),
                    "DLT triangulation");
}

int mvhmr_triangulate_dlt_weighted(const float *proj, const float *points, const float *confidences, float *out, int32_t batch, int32_t views,
                                   int32_t points_per_sample, int32_t confidences_per_sample, void *hip_stream)
{
    if (!proj || !points || !confidences || !out) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (batch < 1 || views < 2) return fail(MVHMR_ERR_INVALID_ARGUMENT, "batch must be >= 1 and views >= 2 (got %d, %d)", batch, views);
    return launched(launch_triangulate_dlt(proj, points, confidences, out, batch, views, points_per_sample ? 1 : 0, confidences_per_sample ? 1 : 0,
                                           static_cast<hipStream_t>(hip_stream)), "weighted DLT triangulation");
}

int mvhmr_triangulate_dlt_backward(const float *proj, const float *points, const float *confidences, const float *grad_out, float *grad_proj,
                                   float *grad_points, float *grad_conf, int32_t batch, int32_t views, int32_t points_per_sample,
                                   int32_t confidences_per_sample, void *hip_stream)
{
    if (!proj || !points || !grad_out) return fail(MVHMR_ERR_INVALID_ARGUMENT, "proj / points / grad_out must be non-null");
    if (!grad_proj && !grad_points && !grad_conf) return fail(MVHMR_ERR_INVALID_ARGUMENT, "grad_proj, grad_points and grad_conf are all null: nothing to compute");
    if (batch < 1 || views < 1) return fail(MVHMR_ERR_INVALID_ARGUMENT, "batch and views must be >= 1 (got %d, %d)", batch, views);
    return launched(launch_triangulate_dlt_bwd(proj, points, confidences, grad_out, grad_proj, grad_points, grad_conf, batch, views, points_per_sample ? 1 : 0,
                                               confidences && confidences_per_sample ? 1 : 0, static_cast<hipStream_t>(hip_stream)),
                    "DLT triangulation backward");
}

int mvhmr_build_coord_volumes(float *coords, const float *rot, const float *center, int32_t batch, int32_t volume_size,
                              const double position[3], const double sides[3], void *hip_stream)
{
    if (!coords || !rot || !center || !position || !sides) return fail(MVHMR_ERR_INVALID_ARGUMENT, "null pointer");
    if (batch < 1 || volume_size < 1) return fail(MVHMR_ERR_INVALID_ARGUMENT, "batch and volume_size must be >= 1");
    return launched(launch_build_coords(coords, rot, center, batch, volume_size, position, sides, static_cast<hipStream_t>(hip_stream)),
                    "coord volume build");
}

// ---- volumetric soft-argmax (soft_argmax3d.hip)
namespace {
struct SaCall { Coords coords; float c2, beta; int X; };

int sa_open(int32_t dtype, const float *coords, const float *rot, const float *center, const double *position, const double *sides, int32_t batch,
            int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, double beta, bool placed, SaCall *out)
{
    if (batch < 1 || joints < 1 || vol_x < 1 || vol_y < 1 || vol_z < 1)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d: every dimension must be >= 1 (B=%d J=%d vol=%dx%dx%d)", batch, joints, vol_x, vol_y, vol_z);
    if ((long long)vol_x * vol_y * vol_z > 0x7fffffffLL || (long long)batch * joints > 0x7fffffffLL)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d: X*Y*Z and B*J must stay below 2^31 (vol=%dx%dx%d, B=%d J=%d)", vol_x, vol_y, vol_z, batch, joints);
    if (dtype < MVHMR_F32 || dtype > MVHMR_BF16) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d: unknown dtype %d", dtype);
    if (!(beta == beta) || beta - beta != 0.0) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d: beta must be finite");
    Problem p{};
    p.X = vol_x; p.Y = vol_y; p.Z = vol_z;
    out->X = vol_x;
    out->beta = (float)beta;
    out->c2 = (float)(beta * 1.4426950408889634);
    if (!placed) { out->coords = Coords{}; return MVHMR_OK; }
    if (coords) { out->coords = coords_from_tensor(coords, p); return MVHMR_OK; }
    return coords_from_cuboid(rot, center, position, sides, p, &out->coords);
}
}  // namespace

int32_t mvhmr_soft_argmax3d_splits(int32_t batch, int32_t joints, int64_t voxels)
{
    if (batch < 1 || joints < 1 || voxels < 1) return 0;
    return sa3d_splits(batch, joints, voxels);
}

size_t mvhmr_soft_argmax3d_workspace_bytes(int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z)
{
    if (batch < 1 || joints < 1 || vol_x < 1 || vol_y < 1 || vol_z < 1) return 0;
    return sa3d_workspace_floats(batch, joints, (long long)vol_x * vol_y * vol_z) * sizeof(float);
}

int mvhmr_soft_argmax3d_forward(const void *volumes, int32_t dtype, const float *coords, const float *rot, const float *center,
                                const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                int32_t vol_z, double beta, float *keypoints, float *logsumexp, float *moment, void *workspace,
                                size_t workspace_bytes, void *hip_stream)
{
    if (!volumes || !keypoints || !logsumexp || !moment) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d: volumes / keypoints / logsumexp / moment must be non-null");
    SaCall c;
    const int rc = sa_open(dtype, coords, rot, center, position, sides, batch, joints, vol_x, vol_y, vol_z, beta, true, &c);
    if (rc != MVHMR_OK) return rc;
    const size_t need = mvhmr_soft_argmax3d_workspace_bytes(batch, joints, vol_x, vol_y, vol_z);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(MVHMR_ERR_WORKSPACE, "soft_argmax3d: workspace of %zu bytes needed, 16-byte aligned (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    return launched(launch_sa3d_forward(volumes, dtype, c.coords, batch, joints, c.X, c.c2, keypoints, logsumexp, moment, static_cast<float *>(workspace),
                                        static_cast<hipStream_t>(hip_stream)), "soft_argmax3d forward");
}

int mvhmr_soft_argmax3d_backward(const void *volumes, int32_t dtype, const float *coords, const float *rot, const float *center,
                                 const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                 int32_t vol_z, double beta, const float *logsumexp, const float *moment, const float *grad_keypoints,
                                 const float *grad_logsumexp, void *grad_volumes, void *hip_stream)
{
    if (!volumes || !logsumexp || !moment || !grad_volumes) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward: volumes / logsumexp / moment / grad_volumes must be non-null");
    if (!grad_keypoints && !grad_logsumexp) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward: grad_keypoints and grad_logsumexp are both null: nothing to compute");
    SaCall c;
    const int rc = sa_open(dtype, coords, rot, center, position, sides, batch, joints, vol_x, vol_y, vol_z, beta, true, &c);
    if (rc != MVHMR_OK) return rc;
    return launched(launch_sa3d_backward(volumes, dtype, c.coords, batch, joints, c.X, c.c2, c.beta, logsumexp, moment, grad_keypoints, grad_logsumexp,
                                         grad_volumes, static_cast<hipStream_t>(hip_stream)), "soft_argmax3d backward");
}

int mvhmr_soft_argmax3d_backward_coords(const void *volumes, int32_t dtype, int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z,
                                        double beta, const float *logsumexp, const float *grad_keypoints, float *grad_coords, void *hip_stream)
{
    if (!volumes || !logsumexp || !grad_keypoints || !grad_coords) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward_coords: null pointer");
    SaCall c;
    const int rc = sa_open(dtype, nullptr, nullptr, nullptr, nullptr, nullptr, batch, joints, vol_x, vol_y, vol_z, beta, false, &c);
    if (rc != MVHMR_OK) return rc;
    return launched(launch_sa3d_backward_coords(volumes, dtype, batch, joints, (long long)vol_x * vol_y * vol_z, c.c2, logsumexp, grad_keypoints, grad_coords,
                                                static_cast<hipStream_t>(hip_stream)), "soft_argmax3d backward_coords");
}

int mvhmr_soft_argmax3d_backward_pose(const float *rot, const float *moment, const float *grad_keypoints, float *grad_rot, float *grad_center,
                                      int32_t batch, int32_t joints, void *hip_stream)
{
    if (!rot || !moment || !grad_keypoints) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward_pose: rot / moment / grad_keypoints must be non-null");
    if (!grad_rot && !grad_center) return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward_pose: grad_rot and grad_center are both null: nothing to compute");
    if (batch < 1 || joints < 1 || (long long)batch * joints > 0x7fffffffLL)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "soft_argmax3d backward_pose: batch and joints must be >= 1 and B*J below 2^31 (got %d, %d)", batch, joints);
    return launched(launch_sa3d_backward_pose(rot, moment, grad_keypoints, grad_rot, grad_center, batch, joints, static_cast<hipStream_t>(hip_stream)),
                    "soft_argmax3d pose gradient");
}

// ---- trilinear volume sampling at world points (volume_sample.hip)
namespace {
int vs_sizes(int32_t dtype, int32_t batch, int32_t channels, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t n_points, int32_t paired)
{
    if (batch < 1 || channels < 1 || n_points < 1)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: batch, channels and points must be >= 1 (B=%d C=%d N=%d)", batch, channels, n_points);
    if (vol_x < 2 || vol_y < 2 || vol_z < 2)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: every extent must be >= 2: a one-voxel axis has no step (vol=%dx%dx%d)", vol_x, vol_y, vol_z);
    if ((long long)vol_x * vol_y * vol_z > 0x7fffffffLL || (long long)batch * channels > 0x7fffffffLL || (long long)batch * n_points > 0x7fffffffLL)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: X*Y*Z, B*C and B*N must stay below 2^31 (vol=%dx%dx%d, B=%d C=%d N=%d)", vol_x, vol_y, vol_z,
                    batch, channels, n_points);
    if (dtype < MVHMR_F32 || dtype > MVHMR_BF16) return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: unknown dtype %d", dtype);
    if (paired != 0 && paired != 1) return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: paired must be 0 or 1, got %d", paired);
    if (paired && n_points != channels)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: a paired call samples channel j at point j and needs N == C (N=%d C=%d)", n_points, channels);
    return MVHMR_OK;
}

int vs_cuboid(const float *rot, const float *center, const double *position, const double *sides, int32_t vol_x, int32_t vol_y, int32_t vol_z, Coords *out)
{
    Problem p{};
    p.X = vol_x; p.Y = vol_y; p.Z = vol_z;
    return coords_from_cuboid(rot, center, position, sides, p, out);
}

int vs_workspace(void *workspace, size_t workspace_bytes, int32_t batch, int32_t n_points)
{
    const size_t need = vs3d_workspace_bytes(batch, n_points);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(MVHMR_ERR_WORKSPACE, "sample_volume: workspace of %zu bytes needed, 16-byte aligned (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    return MVHMR_OK;
}
}  // namespace

int32_t mvhmr_sample_volume_chunk_points(void) { return vs3d_chunk_points(); }

size_t mvhmr_sample_volume_workspace_bytes(int32_t batch, int32_t points)
{
    if (batch < 1 || points < 1) return 0;
    return vs3d_workspace_bytes(batch, points);
}

int mvhmr_sample_volume_forward(const void *volumes, int32_t dtype, const float *points, const float *rot, const float *center,
                                const double position[3], const double sides[3], int32_t batch, int32_t channels, int32_t vol_x, int32_t vol_y,
                                int32_t vol_z, int32_t n_points, int32_t paired, float *samples, float *index, void *hip_stream)
{
    if (!volumes || !points || !samples || !index) return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume: volumes / points / samples / index must be non-null");
    int rc = vs_sizes(dtype, batch, channels, vol_x, vol_y, vol_z, n_points, paired);
    if (rc != MVHMR_OK) return rc;
    Coords cs;
    if ((rc = vs_cuboid(rot, center, position, sides, vol_x, vol_y, vol_z, &cs)) != MVHMR_OK) return rc;
    return launched(launch_vs3d_forward(volumes, dtype, cs, points, batch, channels, vol_x, n_points, paired, samples, index,
                                        static_cast<hipStream_t>(hip_stream)), "sample_volume forward");
}

int mvhmr_sample_volume_backward_volumes(int32_t dtype, const float *index, const float *grad_samples, int32_t batch, int32_t channels,
                                         int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t n_points, int32_t paired, void *grad_volumes,
                                         void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!index || !grad_samples || !grad_volumes) return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume backward_volumes: index / grad_samples / grad_volumes must be non-null");
    int rc = vs_sizes(dtype, batch, channels, vol_x, vol_y, vol_z, n_points, paired);
    if (rc != MVHMR_OK) return rc;
    if ((rc = vs_workspace(workspace, workspace_bytes, batch, n_points)) != MVHMR_OK) return rc;
    return launched(launch_vs3d_backward_volumes(dtype, index, grad_samples, batch, channels, vol_x, vol_y, vol_z, n_points, paired, grad_volumes, workspace,
                                                 static_cast<hipStream_t>(hip_stream)), "sample_volume volume gradient");
}

int mvhmr_sample_volume_backward_geometry(const void *volumes, int32_t dtype, const float *points, const float *rot, const float *center,
                                          const double position[3], const double sides[3], int32_t batch, int32_t channels, int32_t vol_x,
                                          int32_t vol_y, int32_t vol_z, int32_t n_points, int32_t paired, const float *index,
                                          const float *grad_samples, float *grad_points, float *grad_rot, float *grad_center, void *workspace,
                                          size_t workspace_bytes, void *hip_stream)
{
    if (!volumes || !points || !index || !grad_samples)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume backward_geometry: volumes / points / index / grad_samples must be non-null");
    if (!grad_points && !grad_rot && !grad_center)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "sample_volume backward_geometry: grad_points, grad_rot and grad_center are all null: nothing to compute");
    int rc = vs_sizes(dtype, batch, channels, vol_x, vol_y, vol_z, n_points, paired);
    if (rc != MVHMR_OK) return rc;
    Coords cs;
    if ((rc = vs_cuboid(rot, center, position, sides, vol_x, vol_y, vol_z, &cs)) != MVHMR_OK) return rc;
    if ((rc = vs_workspace(workspace, workspace_bytes, batch, n_points)) != MVHMR_OK) return rc;
    return launched(launch_vs3d_backward_geometry(volumes, dtype, cs, points, index, grad_samples, batch, channels, vol_x, n_points, paired, grad_points,
                                                  grad_rot, grad_center, static_cast<float *>(workspace), static_cast<hipStream_t>(hip_stream)),
                    "sample_volume geometry gradient");
}

// ---- ray-marching volumes into camera-view maps (volume_project.hip)
namespace {
int pv_sizes(int32_t dtype, int32_t batch, int32_t views, int32_t channels, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t map_h, int32_t map_w,
             int32_t n_samples, int32_t method, double beta, double min_depth, double max_depth)
{
    if (batch < 1 || views < 1 || channels < 1 || map_h < 1 || map_w < 1)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: batch, views, channels and the map extents must be >= 1 (B=%d V=%d C=%d map=%dx%d)", batch,
                    views, channels, map_h, map_w);
    if (vol_x < 2 || vol_y < 2 || vol_z < 2)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: every extent must be >= 2: a one-voxel axis has no step (vol=%dx%dx%d)", vol_x, vol_y, vol_z);
    if (n_samples < 1 || n_samples > pv3d_max_samples())
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: n_samples must be 1 .. %d, got %d", pv3d_max_samples(), n_samples);
    const long long lim = 0x7fffffffLL, hw = (long long)map_h * map_w, bc = (long long)batch * channels;
    if ((long long)vol_x * vol_y * vol_z > lim || bc > lim || bc * views > lim || hw > lim || hw * views > lim || hw * views * n_samples > lim)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: X*Y*Z, B*C*V and V*Hm*Wm*K must stay below 2^31 (vol=%dx%dx%d, B=%d C=%d V=%d map=%dx%d K=%d)",
                    vol_x, vol_y, vol_z, batch, channels, views, map_h, map_w, n_samples);
    if (dtype < MVHMR_F32 || dtype > MVHMR_BF16) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: unknown dtype %d", dtype);
    if (method < MVHMR_PROJECT_MEAN || method > MVHMR_PROJECT_SOFTMAX) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: unknown method %d", method);
    if (method == MVHMR_PROJECT_SOFTMAX && !(std::isfinite(beta) && (float)beta != 0.f && std::isfinite((float)beta)))
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: beta must be finite and nonzero, got %g", beta);
    if (!std::isfinite(min_depth) || max_depth != max_depth)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: min_depth must be finite and max_depth not NaN (got %g, %g)", min_depth, max_depth);
    return MVHMR_OK;
}
}  // namespace

int32_t mvhmr_project_volume_max_samples(void) { return pv3d_max_samples(); }

void mvhmr_project_volume_channel_group(int32_t group_unroll[2])
{
    int g[2];
    pv3d_channel_group(g);
    if (group_unroll) { group_unroll[0] = g[0]; group_unroll[1] = g[1]; }
}

size_t mvhmr_project_volume_workspace_bytes(int32_t batch, int32_t channels, int32_t vol_x, int32_t vol_y, int32_t vol_z)
{
    if (batch < 1 || channels < 1 || vol_x < 2 || vol_y < 2 || vol_z < 2 || (long long)vol_x * vol_y * vol_z > 0x7fffffffLL) return 0;
    return pv3d_workspace_bytes(batch, channels, (long long)vol_x * vol_y * vol_z);
}

int mvhmr_project_volume_forward(const void *volumes, int32_t dtype, const float *rays, const float *rot, const float *center,
                                 const double position[3], const double sides[3], int32_t batch, int32_t views, int32_t channels, int32_t vol_x,
                                 int32_t vol_y, int32_t vol_z, int32_t map_h, int32_t map_w, int32_t n_samples, int32_t method, double beta,
                                 double min_depth, double max_depth, float *maps, float *ranges, void *aux, void *hip_stream)
{
    if (!volumes || !rays || !maps || !ranges) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: volumes / rays / maps / ranges must be non-null");
    int rc = pv_sizes(dtype, batch, views, channels, vol_x, vol_y, vol_z, map_h, map_w, n_samples, method, beta, min_depth, max_depth);
    if (rc != MVHMR_OK) return rc;
    if (method != MVHMR_PROJECT_MEAN && !aux) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume: max and softmax need aux");
    Coords cs;
    if ((rc = vs_cuboid(rot, center, position, sides, vol_x, vol_y, vol_z, &cs)) != MVHMR_OK) return rc;
    return launched(launch_pv3d_forward(volumes, dtype, cs, rays, batch, views, channels, vol_x, map_h, map_w, n_samples, method, (float)beta,
                                        (float)min_depth, (float)max_depth, maps, ranges, aux, static_cast<hipStream_t>(hip_stream)),
                    "project_volume forward");
}

int mvhmr_project_volume_backward_volumes(const void *volumes, int32_t dtype, const float *rays, const float *rot, const float *center,
                                          const double position[3], const double sides[3], int32_t batch, int32_t views, int32_t channels,
                                          int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t map_h, int32_t map_w, int32_t n_samples,
                                          int32_t method, double beta, double min_depth, double max_depth, const float *grad_maps,
                                          const float *maps, const void *aux, void *grad_volumes, void *workspace, size_t workspace_bytes,
                                          void *hip_stream)
{
    if (!volumes || !rays || !grad_maps || !grad_volumes)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume backward_volumes: volumes / rays / grad_maps / grad_volumes must be non-null");
    int rc = pv_sizes(dtype, batch, views, channels, vol_x, vol_y, vol_z, map_h, map_w, n_samples, method, beta, min_depth, max_depth);
    if (rc != MVHMR_OK) return rc;
    if (method != MVHMR_PROJECT_MEAN && !aux) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume backward_volumes: max and softmax need the forward's aux");
    if (method == MVHMR_PROJECT_SOFTMAX && !maps) return fail(MVHMR_ERR_INVALID_ARGUMENT, "project_volume backward_volumes: softmax needs the forward's maps");
    Coords cs;
    if ((rc = vs_cuboid(rot, center, position, sides, vol_x, vol_y, vol_z, &cs)) != MVHMR_OK) return rc;
    const size_t need = pv3d_workspace_bytes(batch, channels, (long long)vol_x * vol_y * vol_z);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(MVHMR_ERR_WORKSPACE, "project_volume: workspace of %zu bytes needed, 16-byte aligned (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    return launched(launch_pv3d_backward_volumes(volumes, dtype, cs, rays, batch, views, channels, vol_x, map_h, map_w, n_samples, method, (float)beta,
                                                 (float)min_depth, (float)max_depth, grad_maps, maps, aux, grad_volumes, workspace,
                                                 static_cast<hipStream_t>(hip_stream)), "project_volume volume gradient");
}

// ---- 3-D non-maximum suppression and top-K proposals (volume_peaks.hip)
namespace {
int pk_sizes(int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t k)
{
    if (batch < 1 || joints < 1 || vol_x < 1 || vol_y < 1 || vol_z < 1)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: every dimension must be >= 1 (B=%d J=%d vol=%dx%dx%d)", batch, joints, vol_x, vol_y, vol_z);
    const long long lim = 0x7fffffffLL, xy = (long long)vol_x * vol_y;             // stepwise: three 31-bit extents overflow 64 bits
    if (xy > lim || xy * vol_z > lim || (long long)batch * joints > lim)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: X*Y*Z and B*J must stay below 2^31 (vol=%dx%dx%d, B=%d J=%d)", vol_x, vol_y, vol_z, batch, joints);
    if (k < 1 || k > pk3d_max_k()) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: k must be 1 .. %d, got %d", pk3d_max_k(), k);
    return MVHMR_OK;
}

int pk_dtype(int32_t dtype)
{
    if (dtype < MVHMR_F32 || dtype > MVHMR_BF16) return fail(MVHMR_ERR_UNSUPPORTED, "volume_peaks: no kernel for dtype %d", dtype);
    return MVHMR_OK;
}
}  // namespace

void mvhmr_volume_peaks_tile(int32_t tile[3])
{
    int t[3];
    pk3d_tile(t);
    if (tile) { tile[0] = t[0]; tile[1] = t[1]; tile[2] = t[2]; }
}

int32_t mvhmr_volume_peaks_max_k(void) { return pk3d_max_k(); }

size_t mvhmr_volume_peaks_workspace_bytes(int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t k)
{
    if (batch < 1 || joints < 1 || vol_x < 1 || vol_y < 1 || vol_z < 1 || k < 1 || k > pk3d_max_k()) return 0;
    return pk3d_workspace_bytes(batch, joints, vol_x, vol_y, vol_z, k);
}

int mvhmr_volume_peaks(const void *volumes, int32_t dtype, int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y, int32_t vol_z, int32_t k,
                       int32_t radius, float threshold, const float *rot, const float *center, const double position[3], const double sides[3],
                       float *scores, int32_t *index, float *positions, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!volumes || !scores || !index) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: volumes / scores / index must be non-null");
    if (positions && (!rot || !center || !position || !sides))
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: positions need rot / center / position / sides");
    int rc = pk_sizes(batch, joints, vol_x, vol_y, vol_z, k);
    if (rc != MVHMR_OK) return rc;
    if (radius < 0 || radius > 3) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: radius must be 0 .. 3, got %d", radius);
    if (threshold != threshold) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks: threshold must not be NaN");
    if ((rc = pk_dtype(dtype)) != MVHMR_OK) return rc;
    // one launch holds fewer than 2^32 threads along x: 2^24 - 1 blocks of 256 (the launcher applies the same limit)
    if ((long long)batch * joints * pk3d_blocks_per_slice(vol_x, vol_y, vol_z) > (1LL << 24) - 1)
        return fail(MVHMR_ERR_UNSUPPORTED, "volume_peaks: B*J*blocks_per_slice must stay below 2^24 (B=%d J=%d vol=%dx%dx%d): split the batch", batch, joints,
                    vol_x, vol_y, vol_z);
    const size_t need = pk3d_workspace_bytes(batch, joints, vol_x, vol_y, vol_z, k);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(MVHMR_ERR_WORKSPACE, "volume_peaks: workspace of %zu bytes needed, 16-byte aligned (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    Coords cs{};
    if (positions) {
        Problem p{};
        p.X = vol_x; p.Y = vol_y; p.Z = vol_z;
        if ((rc = coords_from_cuboid(rot, center, position, sides, p, &cs)) != MVHMR_OK) return rc;
    }
    return launched(launch_pk3d_forward(volumes, dtype, cs, batch, joints, vol_x, vol_y, vol_z, k, radius, pk3d_key(threshold), scores, index, positions,
                                        workspace, static_cast<hipStream_t>(hip_stream)), "volume_peaks forward");
}

int mvhmr_volume_peaks_backward(int32_t dtype, const int32_t *index, const float *grad_scores, int32_t batch, int32_t joints, int32_t vol_x,
                                int32_t vol_y, int32_t vol_z, int32_t k, void *grad_volumes, void *hip_stream)
{
    if (!index || !grad_scores || !grad_volumes) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks backward: index / grad_scores / grad_volumes must be non-null");
    int rc = pk_sizes(batch, joints, vol_x, vol_y, vol_z, k);
    if (rc != MVHMR_OK) return rc;
    if ((rc = pk_dtype(dtype)) != MVHMR_OK) return rc;
    return launched(launch_pk3d_backward(dtype, index, grad_scores, (long long)batch * joints, (long long)vol_x * vol_y * vol_z, k, grad_volumes,
                                         static_cast<hipStream_t>(hip_stream)), "volume_peaks volume gradient");
}

int mvhmr_volume_peaks_backward_pose(const int32_t *index, const float *grad_positions, const float *rot, const float *center,
                                     const double position[3], const double sides[3], int32_t batch, int32_t joints, int32_t vol_x, int32_t vol_y,
                                     int32_t vol_z, int32_t k, float *grad_rot, float *grad_center, void *hip_stream)
{
    if (!index || !grad_positions || !rot || !center || !position || !sides)
        return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks backward_pose: index / grad_positions / rot / center / position / sides must be non-null");
    if (!grad_rot && !grad_center) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks backward_pose: grad_rot and grad_center are both null: nothing to compute");
    int rc = pk_sizes(batch, joints, vol_x, vol_y, vol_z, k);
    if (rc != MVHMR_OK) return rc;
    if ((long long)joints * k > 0x7fffffffLL) return fail(MVHMR_ERR_INVALID_ARGUMENT, "volume_peaks backward_pose: J*K must stay below 2^31 (J=%d K=%d)", joints, k);
    Coords cs;
    Problem p{};
    p.X = vol_x; p.Y = vol_y; p.Z = vol_z;
    if ((rc = coords_from_cuboid(rot, center, position, sides, p, &cs)) != MVHMR_OK) return rc;
    return launched(launch_pk3d_backward_pose(index, grad_positions, cs, batch, joints, k, grad_rot, grad_center, static_cast<hipStream_t>(hip_stream)),
                    "volume_peaks pose gradient");
}

}  // extern "C"
