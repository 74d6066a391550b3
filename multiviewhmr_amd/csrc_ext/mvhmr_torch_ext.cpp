// PyTorch-ROCm C++ extension over the C ABI (include/mvhmr_unproject.h): the host side of every un-projection launch, as the ops
// mvhmr_native::unprojection[_backward[_geometry]] / unprojection_cuboid[_backward[_geometry]] that multiviewhmr_amd/aggregation.py calls
// from its torch.library ops and from _FusedAggregate, and of the DLT triangulation (triangulate_dlt[_backward], multiview.py).  Every
// un-projection op takes the optional inputs of the call record behind its descriptor fields -- `Tensor? view_mask`, `Tensor? view_weights`,
// `bool visible_only`, `Tensor? view_confidence`, `int moments`, `Tensor? feature_index` ((M,) int32: the volumes' tensors then hold M
// entries), `Tensor? lens` ((B, V, 10) fp32 records) -- the two feature backwards also `bool deterministic`, the geometry ops also
// `Tensor(a!)? grad_weights` and `Tensor(b!)? grad_confidence`, the tensors they write the gradients w.r.t. the weights and the maps into.
// view_args() turns them into one mvhmr_unproject_call and names its family; mvhmr_visibility::view_visibility[_cuboid] return the
// (B, X, Y, Z) int32 bitmask of the views that see each voxel; the tensor and the cuboid form of a call share one body, generic over what
// places the volume.  Per call: tensor checks, descriptor, record, output and workspace from the caching allocator, the current HIP stream,
// one C-ABI call.  mvhmr_softargmax::soft_argmax3d[_cuboid] and their backwards are the volumetric soft-argmax (softargmax.py),
// mvhmr_volsample::sample_volume and its two backwards the trilinear read-back of a volume at world points (volsample.py),
// mvhmr_volproject::project_volume and its backward the ray-march of a volume into camera-view maps (volproject.py),
// mvhmr_peaks::volume_peaks[_cuboid] and their two backwards the 3-D non-maximum suppression with top-K (peaks.py).  Host code only: the
// kernels live in libmvhmr_unproject.so.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "mvhmr_unproject.h"

namespace {

// B..W: the logical feature shape; X..Z: the volume
mvhmr_unproject_desc make_desc(int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t X, int64_t Y, int64_t Z, int64_t method,
                               int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant)
{
    mvhmr_unproject_desc d;
    d.abi_version = MVHMR_ABI_VERSION;
    d.batch = (int32_t)B; d.views = (int32_t)V; d.channels = (int32_t)C; d.feat_h = (int32_t)H; d.feat_w = (int32_t)W;
    d.vol_x = (int32_t)X; d.vol_y = (int32_t)Y; d.vol_z = (int32_t)Z;
    d.method = (int32_t)method; d.feat_dtype = (int32_t)feat_dtype; d.out_dtype = (int32_t)out_dtype;
    d.feat_layout = (int32_t)layout; d.variant = (int32_t)variant;
    return d;
}

// M: the number of volumes (B without a feature_index)
mvhmr_unproject_desc coords_desc(const at::Tensor &coords, int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t method,
                                 int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant, int64_t M = -1)
{
    TORCH_CHECK(coords.dim() == 5 && coords.size(0) == (M < 0 ? B : M) && coords.size(4) == 3, "mvhmr_unproject: coord_volumes must be fp32 (",
                M < 0 || M == B ? "B" : "M", ", X, Y, Z, 3) with ", M < 0 ? B : M, " volumes");
    return make_desc(B, V, C, H, W, coords.size(1), coords.size(2), coords.size(3), method, feat_dtype, out_dtype, layout, variant);
}

mvhmr_unproject_desc cuboid_desc(at::ArrayRef<double> position, at::ArrayRef<double> sides, at::IntArrayRef vol, int64_t B, int64_t V, int64_t C,
                                 int64_t H, int64_t W, int64_t method, int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant)
{
    TORCH_CHECK(position.size() == 3 && sides.size() == 3 && vol.size() == 3, "mvhmr_unproject: position, sides and vol take 3 values each");
    return make_desc(B, V, C, H, W, vol[0], vol[1], vol[2], method, feat_dtype, out_dtype, layout, variant);
}

at::ScalarType scalar_of(int64_t code)
{
    return code == MVHMR_F16 ? at::kHalf : code == MVHMR_BF16 ? at::kBFloat16 : at::kFloat;
}

// a tensor the library reads through a plain pointer: contiguous on the features' device, `dtype` with `numel` elements
void check_tensor(const at::Tensor &t, const at::Tensor &features, const char *name, at::ScalarType dtype, int64_t numel)
{
    TORCH_CHECK(t.is_cuda() && t.device() == features.device() && t.is_contiguous(), "mvhmr_unproject: ", name,
                " must be a contiguous tensor on ", features.device(), ", got one on ", t.device());
    TORCH_CHECK(t.scalar_type() == dtype && t.numel() == numel, "mvhmr_unproject: ", name, " must be ", dtype, " with ", numel,
                " elements, got ", t.scalar_type(), " with ", t.numel());
}

// The C ABI trusts its descriptor (plain pointers carry no sizes): every tensor is checked against it HERE, before anything is launched.
// coords (tensor ops) or rot + center (cuboid ops) describe the volume; grad_out is undefined for a forward.
// M volumes: the tensors that place the volume and grad_out are per volume (M == B without a feature_index)
void check_inputs(const mvhmr_unproject_desc &d, const at::Tensor &features, const at::Tensor &proj, const at::Tensor *coords,
                  const at::Tensor *rot, const at::Tensor *center, const at::Tensor *grad_out, int64_t M, int64_t halves = 1)
{
    const int64_t B = d.batch, V = d.views, C = d.channels, H = d.feat_h, W = d.feat_w;
    const bool shared = M != B;                                 // (the messages name the leading extent the tensor is checked against)
    TORCH_CHECK(features.is_cuda() && features.is_contiguous(), "mvhmr_unproject: features must be a contiguous tensor on a HIP device");
    TORCH_CHECK(B >= 1 && V >= 1 && C >= 1 && H >= 1 && W >= 1, "mvhmr_unproject: every dimension must be >= 1");
    TORCH_CHECK(d.feat_dtype == MVHMR_F32 || d.feat_dtype == MVHMR_F16, "mvhmr_unproject: features are fp32 or fp16");
    const bool quad = d.feat_layout == MVHMR_LAYOUT_QUAD || d.feat_layout == MVHMR_LAYOUT_QUAD_LOG2E;
    const int64_t need = B * V * ((C + 3) / 4 * 4) * H * W * (quad ? 4 : d.feat_dtype == MVHMR_F16 ? 2 : 4);
    const int64_t have = features.numel() * (int64_t)features.element_size();
    TORCH_CHECK(quad || d.feat_layout == MVHMR_LAYOUT_BVHWC ? have >= need : have == B * V * C * H * W * (int64_t)features.element_size(),
                "mvhmr_unproject: features hold ", have, " bytes, the descriptor (", B, ", ", V, ", ", C, ", ", H, ", ", W, ") needs ", need);
    TORCH_CHECK(quad || features.element_size() == (d.feat_dtype == MVHMR_F16 ? 2 : 4), "mvhmr_unproject: feature dtype and descriptor disagree");
    check_tensor(proj, features, "proj_matricies (B, V, 3, 4)", at::kFloat, B * V * 12);
    if (coords)
        check_tensor(*coords, features, shared ? "coord_volumes (M, X, Y, Z, 3)" : "coord_volumes (B, X, Y, Z, 3)", at::kFloat, M * d.vol_x * d.vol_y * d.vol_z * 3);
    if (rot)
        check_tensor(*rot, features, shared ? "rot (M, 3, 3)" : "rot (B, 3, 3)", at::kFloat, M * 9);
    if (center)
        check_tensor(*center, features, shared ? "center (M, 3)" : "center (B, 3)", at::kFloat, M * 3);
    if (grad_out)
        check_tensor(*grad_out, features, shared ? "grad_out (M, C, X, Y, Z)" : "grad_out (B, C, X, Y, Z)", scalar_of(d.out_dtype),
                     M * halves * C * d.vol_x * d.vol_y * d.vol_z);     // (halves: 2 for the mean and the variance of a moments call)
}


// per-sample view masks (mvhmr_unproject_*_masked): view_mask (B, V) uint8 on the features' device, nonzero = present
void check_mask(const mvhmr_unproject_desc &d, const at::Tensor &features, const at::Tensor &mask)
{
    check_tensor(mask, features, "view_mask (B, V)", at::kByte, (int64_t)d.batch * d.views);
}

// the mask the library reads: null for None, which selects the unmasked entry point
const uint8_t *mask_ptr(const mvhmr_unproject_desc &d, const at::Tensor &features, const c10::optional<at::Tensor> &view_mask)
{
    if (!view_mask || !view_mask->defined()) return nullptr;
    check_mask(d, features, *view_mask);
    return view_mask->data_ptr<uint8_t>();
}

// per-view confidence weights (mvhmr_unproject_*_weighted): view_weights (B, V) fp32 on the features' device; null for None
const float *weights_ptr(const mvhmr_unproject_desc &d, const at::Tensor &features, const c10::optional<at::Tensor> &view_weights, const char *name = "view_weights (B, V)")
{
    if (!view_weights || !view_weights->defined()) return nullptr;
    check_tensor(*view_weights, features, name, at::kFloat, (int64_t)d.batch * d.views);
    return view_weights->data_ptr<float>();
}

// the channels of out / grad_out per feature channel: 2 for the mean and the variance
int64_t halves_of(int64_t moments) { return moments == MVHMR_MOMENTS_MEANVAR ? 2 : 1; }

// shared feature maps (mvhmr_unproject_*_shared): feature_index (M,) int32 on the features' device; null for None
int64_t volumes_of(const c10::optional<at::Tensor> &feature_index, int64_t B)
{
    return feature_index && feature_index->defined() ? feature_index->numel() : B;
}

// per-pixel confidence maps (mvhmr_unproject_*_confidence): (B, V, Hf, Wf) fp32 on the features' device; null for None
const float *confidence_ptr(const mvhmr_unproject_desc &d, const at::Tensor &features, const c10::optional<at::Tensor> &t, const char *name)
{
    if (!t || !t->defined()) return nullptr;
    check_tensor(*t, features, name, at::kFloat, (int64_t)d.batch * d.views * d.feat_h * d.feat_w);
    return t->data_ptr<float>();
}

// the call record of an op: its optional inputs checked against the descriptor, and the family they name -- the one place that chooses it.
// The library refuses the selections a family carries without taking them (a mask beside a lens ...), each with its own text.
mvhmr_unproject_call view_args(const mvhmr_unproject_desc &d, const at::Tensor &features, const c10::optional<at::Tensor> &view_mask,
                               const c10::optional<at::Tensor> &view_weights, bool visible_only, const c10::optional<at::Tensor> &view_confidence,
                               const c10::optional<at::Tensor> &feature_index, const c10::optional<at::Tensor> &lens, int64_t moments)
{
    mvhmr_unproject_call c{};
    c.struct_size = sizeof(c);
    c.view_mask = mask_ptr(d, features, view_mask);
    c.view_weights = weights_ptr(d, features, view_weights);
    c.visible = visible_only;
    c.view_confidence = confidence_ptr(d, features, view_confidence, "view_confidence (B, V, Hf, Wf)");
    if (feature_index && feature_index->defined()) {
        TORCH_CHECK(feature_index->dim() == 1 && feature_index->numel() >= 1 && feature_index->numel() <= INT32_MAX,
                    "mvhmr_unproject: feature_index must be a non-empty (M,) tensor");
        check_tensor(*feature_index, features, "feature_index (M,)", at::kInt, feature_index->numel());
        c.feature_index = feature_index->data_ptr<int32_t>();
        c.volumes = (int32_t)feature_index->numel();
    }
    if (lens && lens->defined()) {
        check_tensor(*lens, features, "lens (B, V, 10)", at::kFloat, (int64_t)d.batch * d.views * 10);
        c.lens = lens->data_ptr<float>();
    }
    c.moments = (int32_t)moments;
    TORCH_CHECK(!moments || (!c.view_weights && !c.view_confidence && !c.feature_index && !c.lens),
                "mvhmr_unproject: the cross-view variance takes a view mask and visible_only only (view_weights, view_confidence, feature_index and lens are not built yet)");
    TORCH_CHECK(!(c.visible && c.view_weights), "mvhmr_unproject: visible_only does not take view_weights");
    TORCH_CHECK(!(c.view_confidence && c.view_weights), "mvhmr_unproject: view_confidence does not take view_weights");
    c.family = c.moments           ? MVHMR_FAMILY_MOMENTS
               : c.lens            ? MVHMR_FAMILY_LENS
               : c.feature_index   ? MVHMR_FAMILY_SHARED
               : c.view_confidence ? MVHMR_FAMILY_CONFIDENCE
               : c.visible         ? MVHMR_FAMILY_VISIBLE
               : c.view_weights    ? MVHMR_FAMILY_WEIGHTED
               : c.view_mask       ? MVHMR_FAMILY_MASKED
                                   : MVHMR_FAMILY_PLAIN;
    return c;
}

// the common tail: workspace, the features' device, the current HIP stream, one C-ABI call.  The workspace comes from the caching
// allocator through at::empty -- except `unfilled` (the deterministic entry points), straight from the device allocator: under
// torch.use_deterministic_algorithms(True) at::empty fills new memory (torch.utils.deterministic.fill_uninitialized_memory) --
// gigabytes of scratch the kernels overwrite or clear themselves
template <typename Launch>
void run(const at::Tensor &features, const mvhmr_unproject_desc &d, const mvhmr_unproject_call &c, mvhmr_call_kind_t kind, Launch launch)
{
    const size_t need = mvhmr_unproject_call_workspace_bytes(&d, &c, kind);
    const bool unfilled = kind == MVHMR_CALL_BACKWARD && c.deterministic;
    c10::DeviceGuard guard(features.device());
    c10::DataPtr raw;
    at::Tensor filled;
    if (unfilled) raw = c10::GetAllocator(features.device().type())->allocate(need);
    else filled = at::empty({(int64_t)need}, features.options().dtype(at::kByte));
    void *ws = unfilled ? raw.get() : filled.data_ptr();
    const int status = launch(&d, &c, need ? ws : nullptr, need, c10::hip::getCurrentHIPStream(features.device().index()).stream());
    TORCH_CHECK(status == MVHMR_OK, "mvhmr_unproject: ", mvhmr_last_error());
}

// gradient w.r.t. the features in their dtype: channels-last strides for channels-last features (the permuted view's data_ptr() is
// its storage's), planar otherwise, quad-planar features included
at::Tensor new_feature_grad(const mvhmr_unproject_desc &d, const at::Tensor &features)
{
    const auto opts = features.options().dtype(scalar_of(d.feat_dtype));
    if (d.feat_layout == MVHMR_LAYOUT_BVHWC)
        return at::empty({d.batch, d.views, d.feat_h, d.feat_w, d.channels}, opts).permute({0, 1, 4, 2, 3});
    return at::empty({d.batch, d.views, d.channels, d.feat_h, d.feat_w}, opts);
}

// the descriptor's fields as the ops take them: B..W the logical feature shape
struct DescArgs {
    int64_t B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant;
    int64_t M;                                                  // volumes: B, or the length of the feature_index
};

// ---- what places the volume.  Each form knows its descriptor, its tensors' checks, the shapes of its geometry gradients, the placing
// fields and geometry outputs of the call record, and its visibility call.
struct TensorVolume {
    const at::Tensor &coords;                                   // (B, X, Y, Z, 3)
    static constexpr const char *kNothingAsked = "mvhmr_unproject: neither gradient was asked for";

    mvhmr_unproject_desc desc(const DescArgs &a) const
    {
        return coords_desc(coords, a.B, a.V, a.C, a.H, a.W, a.method, a.feat_dtype, a.out_dtype, a.layout, a.variant, a.M);
    }
    void check(const mvhmr_unproject_desc &d, const at::Tensor &features, const at::Tensor &proj, const at::Tensor *grad_out, int64_t M, int64_t halves) const
    {
        check_inputs(d, features, proj, &coords, nullptr, nullptr, grad_out, M, halves);
    }
    int visibility(const mvhmr_unproject_desc &d, const float *proj, const uint8_t *mask, int32_t *bits, hipStream_t s) const
    {
        return mvhmr_unproject_visibility(&d, proj, coords.data_ptr<float>(), mask, bits, s);
    }
    // gradients w.r.t. proj (B,V,3,4) and coords (B,X,Y,Z,3)
    std::vector<std::vector<int64_t>> geometry_shapes(const mvhmr_unproject_desc &d) const { return {{d.batch, d.views, 3, 4}, coords.sizes().vec()}; }

    void place(mvhmr_unproject_call &c) const
    {
        c.placing = MVHMR_PLACING_TENSOR;
        c.coords = coords.data_ptr<float>();
    }
    void geometry_outputs(mvhmr_unproject_call &c, float *const *g) const { c.grad_proj = g[0]; c.grad_coords = g[1]; }
};

// the cuboid recipe (mvhmr_unproject_*_cuboid): rot (B,3,3) and center (B,3) on the device, position / sides / vol 3 values each
struct CuboidVolume {
    const at::Tensor &rot, &center;
    at::ArrayRef<double> position, sides;
    at::IntArrayRef vol;
    static constexpr const char *kNothingAsked = "mvhmr_unproject: no gradient was asked for";

    mvhmr_unproject_desc desc(const DescArgs &a) const
    {
        return cuboid_desc(position, sides, vol, a.B, a.V, a.C, a.H, a.W, a.method, a.feat_dtype, a.out_dtype, a.layout, a.variant);
    }
    void check(const mvhmr_unproject_desc &d, const at::Tensor &features, const at::Tensor &proj, const at::Tensor *grad_out, int64_t M, int64_t halves) const
    {
        check_inputs(d, features, proj, nullptr, &rot, &center, grad_out, M, halves);
    }
    int visibility(const mvhmr_unproject_desc &d, const float *proj, const uint8_t *mask, int32_t *bits, hipStream_t s) const
    {
        return mvhmr_unproject_visibility_cuboid(&d, proj, rot.data_ptr<float>(), center.data_ptr<float>(), position.data(), sides.data(), mask, bits, s);
    }
    // gradients w.r.t. proj (B,V,3,4), rot (B,3,3) and center (B,3) -- (M,3,3) and (M,3) under a feature_index
    std::vector<std::vector<int64_t>> geometry_shapes(const mvhmr_unproject_desc &d) const { return {{d.batch, d.views, 3, 4}, rot.sizes().vec(), center.sizes().vec()}; }

    void place(mvhmr_unproject_call &c) const
    {
        c.placing = MVHMR_PLACING_CUBOID;
        c.rot = rot.data_ptr<float>();
        c.center = center.data_ptr<float>();
        c.position = position.data();
        c.sides = sides.data();
    }
    void geometry_outputs(mvhmr_unproject_call &c, float *const *g) const { c.grad_proj = g[0]; c.grad_rot = g[1]; c.grad_center = g[2]; }
};

// ---- one body per kind of call.  features: the tensor the library reads (planar, channels-last or the quad-planar byte buffer)
template <typename Volume>
at::Tensor forward(const Volume &vol, const at::Tensor &features, const at::Tensor &proj, const DescArgs &a, const c10::optional<at::Tensor> &view_mask,
                   const c10::optional<at::Tensor> &view_weights, bool visible_only, const c10::optional<at::Tensor> &view_confidence,
                   const c10::optional<at::Tensor> &feature_index, const c10::optional<at::Tensor> &lens, int64_t moments)
{
    const mvhmr_unproject_desc d = vol.desc(a);
    vol.check(d, features, proj, nullptr, a.M, halves_of(moments));
    mvhmr_unproject_call c = view_args(d, features, view_mask, view_weights, visible_only, view_confidence, feature_index, lens, moments);
    at::Tensor out = at::empty({a.M, halves_of(moments) * a.C, d.vol_x, d.vol_y, d.vol_z}, features.options().dtype(scalar_of(a.out_dtype)));
    vol.place(c);
    c.features = features.data_ptr();
    c.proj = proj.data_ptr<float>();
    c.out = out.data_ptr();
    run(features, d, c, MVHMR_CALL_FORWARD, mvhmr_unproject_forward_call);
    return out;
}

// deterministic: the feature gradient bitwise reproducible (mvhmr_unproject_backward*_deterministic); the workspace is not filled
template <typename Volume>
at::Tensor backward(const Volume &vol, const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj, const DescArgs &a,
                    const c10::optional<at::Tensor> &view_mask, bool deterministic, const c10::optional<at::Tensor> &view_weights, bool visible_only,
                    const c10::optional<at::Tensor> &view_confidence, const c10::optional<at::Tensor> &feature_index,
                    const c10::optional<at::Tensor> &lens, int64_t moments)
{
    const mvhmr_unproject_desc d = vol.desc(a);
    vol.check(d, features, proj, &grad_out, a.M, halves_of(moments));
    mvhmr_unproject_call c = view_args(d, features, view_mask, view_weights, visible_only, view_confidence, feature_index, lens, moments);
    at::Tensor grad = new_feature_grad(d, features);
    vol.place(c);
    c.deterministic = deterministic;
    c.grad_out = grad_out.data_ptr();
    c.features = features.data_ptr();
    c.proj = proj.data_ptr<float>();
    c.grad_features = grad.data_ptr();
    run(features, d, c, MVHMR_CALL_BACKWARD, mvhmr_unproject_backward_call);
    return grad;
}

// the geometry gradients of the form, all fp32, grad_proj first; an output not asked for comes back as an empty tensor.  grad_weights, when
// given (with view_weights), is written in place: the gradient w.r.t. the weights, which may be the only one asked for
template <typename Volume>
std::vector<at::Tensor> backward_geometry(const Volume &vol, const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj, const DescArgs &a,
                                          std::initializer_list<bool> want, const c10::optional<at::Tensor> &view_mask,
                                          const c10::optional<at::Tensor> &view_weights, const c10::optional<at::Tensor> &grad_weights, bool visible_only,
                                          const c10::optional<at::Tensor> &view_confidence, const c10::optional<at::Tensor> &grad_confidence,
                                          const c10::optional<at::Tensor> &feature_index, const c10::optional<at::Tensor> &lens, int64_t moments)
{
    const bool want_weights = grad_weights && grad_weights->defined();
    const bool want_conf = grad_confidence && grad_confidence->defined();
    TORCH_CHECK(want_weights || want_conf || std::any_of(want.begin(), want.end(), [](bool w) { return w; }), Volume::kNothingAsked);
    const mvhmr_unproject_desc d = vol.desc(a);
    vol.check(d, features, proj, &grad_out, a.M, halves_of(moments));
    mvhmr_unproject_call c = view_args(d, features, view_mask, view_weights, visible_only, view_confidence, feature_index, lens, moments);
    TORCH_CHECK(!want_weights || c.view_weights, "mvhmr_unproject: grad_weights needs view_weights");
    TORCH_CHECK(!want_conf || c.view_confidence, "mvhmr_unproject: grad_confidence needs view_confidence");
    c.grad_weights = const_cast<float *>(weights_ptr(d, features, grad_weights, "grad_weights (B, V)"));
    c.grad_confidence = const_cast<float *>(confidence_ptr(d, features, grad_confidence, "grad_confidence (B, V, Hf, Wf)"));
    const auto opts = features.options().dtype(at::kFloat);
    const auto shapes = vol.geometry_shapes(d);
    std::vector<at::Tensor> grads;
    std::vector<float *> ptrs;
    for (size_t i = 0; i < shapes.size(); i++) {
        const bool w = want.begin()[i];
        grads.push_back(w ? at::empty(shapes[i], opts) : at::empty({0}, opts));
        ptrs.push_back(w ? grads.back().data_ptr<float>() : nullptr);
    }
    vol.place(c);
    vol.geometry_outputs(c, ptrs.data());
    c.grad_out = grad_out.data_ptr();
    c.features = features.data_ptr();
    c.proj = proj.data_ptr<float>();
    run(features, d, c, MVHMR_CALL_GEOMETRY, mvhmr_unproject_backward_geometry_call);
    return grads;
}

// the (B, X, Y, Z) int32 bitmask of the views that are present and see each voxel: proj is the tensor every other one is checked against
template <typename Volume>
at::Tensor visibility(const Volume &vol, const at::Tensor &proj, const mvhmr_unproject_desc &d, const c10::optional<at::Tensor> &view_mask)
{
    TORCH_CHECK(proj.is_cuda() && proj.is_contiguous() && proj.scalar_type() == at::kFloat && proj.numel() == (int64_t)d.batch * d.views * 12,
                "mvhmr_unproject: proj_matricies must be a contiguous fp32 (B, V, 3, 4) tensor on a HIP device");
    const uint8_t *mask = mask_ptr(d, proj, view_mask);
    c10::DeviceGuard guard(proj.device());
    at::Tensor bits = at::empty({d.batch, d.vol_x, d.vol_y, d.vol_z}, proj.options().dtype(at::kInt));
    const int status = vol.visibility(d, proj.data_ptr<float>(), mask, bits.data_ptr<int32_t>(), c10::hip::getCurrentHIPStream(proj.device().index()).stream());
    TORCH_CHECK(status == MVHMR_OK, "mvhmr_unproject: ", mvhmr_last_error());
    return bits;
}

// ---- the ops
using OptTensor = c10::optional<at::Tensor>;

at::Tensor view_visibility_native(const at::Tensor &proj, const at::Tensor &coords, int64_t H, int64_t W, const OptTensor &view_mask)
{
    const int64_t B = proj.size(0), V = proj.size(1);
    const mvhmr_unproject_desc d = coords_desc(coords, B, V, 1, H, W, MVHMR_AGG_SUM, MVHMR_F32, MVHMR_F32, MVHMR_LAYOUT_BVCHW, MVHMR_VARIANT_AUTO);
    check_tensor(coords, proj, "coord_volumes (B, X, Y, Z, 3)", at::kFloat, B * d.vol_x * d.vol_y * d.vol_z * 3);
    return visibility(TensorVolume{coords}, proj, d, view_mask);
}

at::Tensor view_visibility_cuboid_native(const at::Tensor &proj, const at::Tensor &rot, const at::Tensor &center, at::ArrayRef<double> position,
                                         at::ArrayRef<double> sides, at::IntArrayRef vol, int64_t H, int64_t W, const OptTensor &view_mask)
{
    const int64_t B = proj.size(0), V = proj.size(1);
    const mvhmr_unproject_desc d = cuboid_desc(position, sides, vol, B, V, 1, H, W, MVHMR_AGG_SUM, MVHMR_F32, MVHMR_F32, MVHMR_LAYOUT_BVCHW, MVHMR_VARIANT_AUTO);
    check_tensor(rot, proj, "rot (B, 3, 3)", at::kFloat, B * 9);
    check_tensor(center, proj, "center (B, 3)", at::kFloat, B * 3);
    return visibility(CuboidVolume{rot, center, position, sides, vol}, proj, d, view_mask);
}

at::Tensor unprojection_native(const at::Tensor &features, const at::Tensor &proj, const at::Tensor &coords, int64_t B, int64_t V, int64_t C,
                               int64_t H, int64_t W, int64_t method, int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant,
                               const OptTensor &view_mask, const OptTensor &view_weights, bool visible_only, const OptTensor &view_confidence,
                               int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    return forward(TensorVolume{coords}, features, proj, DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)}, view_mask, view_weights,
                   visible_only, view_confidence, feature_index, lens, moments);
}

at::Tensor unprojection_backward_native(const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj, const at::Tensor &coords,
                                        int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t method, int64_t feat_dtype,
                                        int64_t out_dtype, int64_t layout, int64_t variant, const OptTensor &view_mask, bool deterministic,
                                        const OptTensor &view_weights, bool visible_only, const OptTensor &view_confidence, int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    return backward(TensorVolume{coords}, grad_out, features, proj, DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)}, view_mask,
                    deterministic, view_weights, visible_only, view_confidence, feature_index, lens, moments);
}

std::tuple<at::Tensor, at::Tensor> unprojection_backward_geometry_native(const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj,
                                                                          const at::Tensor &coords, int64_t B, int64_t V, int64_t C, int64_t H,
                                                                          int64_t W, int64_t method, int64_t feat_dtype, int64_t out_dtype, int64_t layout,
                                                                          int64_t variant, bool want_proj, bool want_coords, const OptTensor &view_mask,
                                                                          const OptTensor &view_weights, const OptTensor &grad_weights, bool visible_only,
                                                                          const OptTensor &view_confidence, const OptTensor &grad_confidence,
                                                                          int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    const auto g = backward_geometry(TensorVolume{coords}, grad_out, features, proj, DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)},
                                     {want_proj, want_coords}, view_mask, view_weights, grad_weights, visible_only, view_confidence, grad_confidence, feature_index, lens, moments);
    return {g[0], g[1]};
}

at::Tensor unprojection_cuboid_native(const at::Tensor &features, const at::Tensor &proj, const at::Tensor &rot, const at::Tensor &center,
                                      at::ArrayRef<double> position, at::ArrayRef<double> sides, at::IntArrayRef vol, int64_t B, int64_t V, int64_t C,
                                      int64_t H, int64_t W, int64_t method, int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant,
                                      const OptTensor &view_mask, const OptTensor &view_weights, bool visible_only, const OptTensor &view_confidence,
                                      int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    return forward(CuboidVolume{rot, center, position, sides, vol}, features, proj, DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)},
                   view_mask, view_weights, visible_only, view_confidence, feature_index, lens, moments);
}

at::Tensor unprojection_cuboid_backward_native(const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj, const at::Tensor &rot,
                                               const at::Tensor &center, at::ArrayRef<double> position, at::ArrayRef<double> sides,
                                               at::IntArrayRef vol, int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t method,
                                               int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant, const OptTensor &view_mask,
                                               bool deterministic, const OptTensor &view_weights, bool visible_only, const OptTensor &view_confidence,
                                               int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    return backward(CuboidVolume{rot, center, position, sides, vol}, grad_out, features, proj,
                    DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)}, view_mask, deterministic, view_weights, visible_only, view_confidence, feature_index, lens, moments);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> unprojection_cuboid_backward_geometry_native(
    const at::Tensor &grad_out, const at::Tensor &features, const at::Tensor &proj, const at::Tensor &rot, const at::Tensor &center,
    at::ArrayRef<double> position, at::ArrayRef<double> sides, at::IntArrayRef vol, int64_t B, int64_t V, int64_t C, int64_t H, int64_t W,
    int64_t method, int64_t feat_dtype, int64_t out_dtype, int64_t layout, int64_t variant, bool want_proj, bool want_rot, bool want_center,
    const OptTensor &view_mask, const OptTensor &view_weights, const OptTensor &grad_weights, bool visible_only, const OptTensor &view_confidence,
    const OptTensor &grad_confidence, int64_t moments, const OptTensor &feature_index, const OptTensor &lens)
{
    const auto g = backward_geometry(CuboidVolume{rot, center, position, sides, vol}, grad_out, features, proj,
                                     DescArgs{B, V, C, H, W, method, feat_dtype, out_dtype, layout, variant, volumes_of(feature_index, B)}, {want_proj, want_rot, want_center}, view_mask,
                                     view_weights, grad_weights, visible_only, view_confidence, grad_confidence, feature_index, lens, moments);
    return {g[0], g[1], g[2]};
}

// DLT triangulation (mvhmr_triangulate_dlt[_weighted]) and its backward: proj (B,V,3,4), points (V,2) or (B,V,2), confidences (V) or
// (B,V) or undefined, all fp32 and contiguous on proj's device (the same check and tail as the un-projection ops, proj in the features' place)
void check_dlt(const at::Tensor &proj, const at::Tensor &points, const c10::optional<at::Tensor> &conf, int64_t *B, int64_t *V)
{
    TORCH_CHECK(proj.is_cuda() && proj.is_contiguous() && proj.dim() == 4 && proj.size(2) == 3 && proj.size(3) == 4 && proj.scalar_type() == at::kFloat,
                "mvhmr_triangulate_dlt: proj_matricies must be a contiguous fp32 (B, V, 3, 4) tensor on a HIP device");
    *B = proj.size(0);
    *V = proj.size(1);
    TORCH_CHECK(points.dim() == 2 || points.dim() == 3, "mvhmr_triangulate_dlt: points must be (V, 2) or (B, V, 2)");
    check_tensor(points, proj, "points (V, 2) / (B, V, 2)", at::kFloat, (points.dim() == 3 ? *B : 1) * *V * 2);
    if (conf && conf->defined()) {
        TORCH_CHECK(conf->dim() == 1 || conf->dim() == 2, "mvhmr_triangulate_dlt: confidences must be (V,) or (B, V)");
        check_tensor(*conf, proj, "confidences (V,) / (B, V)", at::kFloat, (conf->dim() == 2 ? *B : 1) * *V);
    }
}

void check_status(int status)
{
    TORCH_CHECK(status == MVHMR_OK, "mvhmr_unproject: ", mvhmr_last_error());
}

at::Tensor triangulate_dlt_native(const at::Tensor &proj, const at::Tensor &points, const c10::optional<at::Tensor> &conf)
{
    int64_t B, V;
    check_dlt(proj, points, conf, &B, &V);
    c10::DeviceGuard guard(proj.device());
    at::Tensor out = at::empty({B, 3}, proj.options());
    const hipStream_t s = c10::hip::getCurrentHIPStream(proj.device().index()).stream();
    const int pps = points.dim() == 3 ? 1 : 0;
    if (conf && conf->defined())
        check_status(mvhmr_triangulate_dlt_weighted(proj.data_ptr<float>(), points.data_ptr<float>(), conf->data_ptr<float>(), out.data_ptr<float>(),
                                                    (int32_t)B, (int32_t)V, pps, conf->dim() == 2 ? 1 : 0, s));
    else
        check_status(mvhmr_triangulate_dlt(proj.data_ptr<float>(), points.data_ptr<float>(), out.data_ptr<float>(), (int32_t)B, (int32_t)V, pps, s));
    return out;
}

// per-sample gradients: grad_proj (B,V,3,4), grad_points (B,V,2), grad_conf (B,V) (the caller sums shared points / confidences)
std::tuple<at::Tensor, at::Tensor, at::Tensor> triangulate_dlt_backward_native(const at::Tensor &grad_out, const at::Tensor &proj, const at::Tensor &points,
                                                                                const c10::optional<at::Tensor> &conf)
{
    int64_t B, V;
    check_dlt(proj, points, conf, &B, &V);
    check_tensor(grad_out, proj, "grad_out (B, 3)", at::kFloat, B * 3);
    c10::DeviceGuard guard(proj.device());
    at::Tensor gp = at::empty({B, V, 3, 4}, proj.options()), gu = at::empty({B, V, 2}, proj.options()), gc = at::empty({B, V}, proj.options());
    const bool weighted = conf && conf->defined();
    check_status(mvhmr_triangulate_dlt_backward(proj.data_ptr<float>(), points.data_ptr<float>(), weighted ? conf->data_ptr<float>() : nullptr,
                                                grad_out.data_ptr<float>(), gp.data_ptr<float>(), gu.data_ptr<float>(), gc.data_ptr<float>(), (int32_t)B,
                                                (int32_t)V, points.dim() == 3 ? 1 : 0, weighted && conf->dim() == 2 ? 1 : 0,
                                                c10::hip::getCurrentHIPStream(proj.device().index()).stream()));
    return {gp, gu, gc};
}

// Volumetric soft-argmax (mvhmr_soft_argmax3d_*; multiviewhmr_amd/softargmax.py): volumes (B,J,X,Y,Z) fp32 / fp16 / bf16, every other tensor
// fp32; the tensor route places the voxels by coords (B,X,Y,Z,3), the cuboid route by rot (B,3,3), center (B,3), position, sides.  The same
// per-call tail as above: checks, outputs and workspace from the caching allocator, the current stream, one C-ABI call.
struct SaPlace {
    const float *coords = nullptr, *rot = nullptr, *center = nullptr;
    const double *position = nullptr, *sides = nullptr;
};

int32_t sa_dtype(const at::Tensor &volumes)
{
    const at::ScalarType t = volumes.scalar_type();
    TORCH_CHECK(t == at::kFloat || t == at::kHalf || t == at::kBFloat16, "mvhmr_soft_argmax3d: volumes must be fp32, fp16 or bf16, got ", t);
    return t == at::kHalf ? MVHMR_F16 : t == at::kBFloat16 ? MVHMR_BF16 : MVHMR_F32;
}

void sa_check_volumes(const at::Tensor &volumes)
{
    TORCH_CHECK(volumes.is_cuda() && volumes.is_contiguous() && volumes.dim() == 5 && volumes.numel() > 0,
                "mvhmr_soft_argmax3d: volumes must be a contiguous, non-empty (B, J, X, Y, Z) tensor on a HIP device");
    TORCH_CHECK(volumes.size(2) * volumes.size(3) * volumes.size(4) < (int64_t(1) << 31) && volumes.size(0) * volumes.size(1) < (int64_t(1) << 31),
                "mvhmr_soft_argmax3d: X*Y*Z and B*J must stay below 2^31");
}

SaPlace sa_place(const at::Tensor &volumes, const at::Tensor *coords, const at::Tensor *rot, const at::Tensor *center, at::ArrayRef<double> position,
                 at::ArrayRef<double> sides)
{
    sa_check_volumes(volumes);
    const int64_t B = volumes.size(0), N = volumes.size(2) * volumes.size(3) * volumes.size(4);
    SaPlace p;
    if (coords) {
        TORCH_CHECK(coords->dim() == 5 && coords->size(0) == B && coords->size(1) == volumes.size(2) && coords->size(2) == volumes.size(3) &&
                    coords->size(3) == volumes.size(4) && coords->size(4) == 3, "mvhmr_soft_argmax3d: coord_volumes must be (B, X, Y, Z, 3) of the volumes' extents");
        check_tensor(*coords, volumes, "coord_volumes (B, X, Y, Z, 3)", at::kFloat, B * N * 3);
        p.coords = coords->data_ptr<float>();
    } else {
        TORCH_CHECK(position.size() == 3 && sides.size() == 3, "mvhmr_soft_argmax3d: position and sides take 3 values each");
        check_tensor(*rot, volumes, "rotations (B, 3, 3)", at::kFloat, B * 9);
        check_tensor(*center, volumes, "centers (B, 3)", at::kFloat, B * 3);
        p.rot = rot->data_ptr<float>(); p.center = center->data_ptr<float>(); p.position = position.data(); p.sides = sides.data();
    }
    return p;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> sa_forward(const at::Tensor &volumes, const SaPlace &p, double beta)
{
    const int64_t B = volumes.size(0), J = volumes.size(1), X = volumes.size(2), Y = volumes.size(3), Z = volumes.size(4);
    c10::DeviceGuard guard(volumes.device());
    const auto f32 = volumes.options().dtype(at::kFloat);
    at::Tensor kp = at::empty({B, J, 3}, f32), lse = at::empty({B, J}, f32), mom = at::empty({B, J, 3}, f32);
    const size_t need = mvhmr_soft_argmax3d_workspace_bytes((int32_t)B, (int32_t)J, (int32_t)X, (int32_t)Y, (int32_t)Z);
    at::Tensor ws = at::empty({(int64_t)need}, volumes.options().dtype(at::kByte));
    check_status(mvhmr_soft_argmax3d_forward(volumes.data_ptr(), sa_dtype(volumes), p.coords, p.rot, p.center, p.position, p.sides, (int32_t)B, (int32_t)J,
                                             (int32_t)X, (int32_t)Y, (int32_t)Z, beta, kp.data_ptr<float>(), lse.data_ptr<float>(), mom.data_ptr<float>(),
                                             ws.data_ptr(), need, c10::hip::getCurrentHIPStream(volumes.device().index()).stream()));
    return {kp, lse, mom};
}

at::Tensor sa_backward(const at::Tensor &volumes, const SaPlace &p, double beta, const at::Tensor &lse, const at::Tensor &moment,
                       const c10::optional<at::Tensor> &grad_kp, const c10::optional<at::Tensor> &grad_lse)
{
    const int64_t B = volumes.size(0), J = volumes.size(1), X = volumes.size(2), Y = volumes.size(3), Z = volumes.size(4);
    check_tensor(lse, volumes, "logsumexp (B, J)", at::kFloat, B * J);
    check_tensor(moment, volumes, "moment (B, J, 3)", at::kFloat, B * J * 3);
    const bool has_k = grad_kp && grad_kp->defined(), has_l = grad_lse && grad_lse->defined();
    TORCH_CHECK(has_k || has_l, "mvhmr_soft_argmax3d: the backward needs grad_keypoints or grad_logsumexp");
    if (has_k) check_tensor(*grad_kp, volumes, "grad_keypoints (B, J, 3)", at::kFloat, B * J * 3);
    if (has_l) check_tensor(*grad_lse, volumes, "grad_logsumexp (B, J)", at::kFloat, B * J);
    c10::DeviceGuard guard(volumes.device());
    at::Tensor gv = at::empty_like(volumes);
    check_status(mvhmr_soft_argmax3d_backward(volumes.data_ptr(), sa_dtype(volumes), p.coords, p.rot, p.center, p.position, p.sides, (int32_t)B, (int32_t)J,
                                              (int32_t)X, (int32_t)Y, (int32_t)Z, beta, lse.data_ptr<float>(), moment.data_ptr<float>(),
                                              has_k ? grad_kp->data_ptr<float>() : nullptr, has_l ? grad_lse->data_ptr<float>() : nullptr, gv.data_ptr(),
                                              c10::hip::getCurrentHIPStream(volumes.device().index()).stream()));
    return gv;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> soft_argmax3d_native(const at::Tensor &volumes, const at::Tensor &coords, double beta)
{
    return sa_forward(volumes, sa_place(volumes, &coords, nullptr, nullptr, {}, {}), beta);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> soft_argmax3d_cuboid_native(const at::Tensor &volumes, const at::Tensor &rot, const at::Tensor &center,
                                                                           at::ArrayRef<double> position, at::ArrayRef<double> sides, double beta)
{
    return sa_forward(volumes, sa_place(volumes, nullptr, &rot, &center, position, sides), beta);
}

at::Tensor soft_argmax3d_backward_native(const at::Tensor &volumes, const at::Tensor &coords, double beta, const at::Tensor &lse, const at::Tensor &moment,
                                         const c10::optional<at::Tensor> &grad_kp, const c10::optional<at::Tensor> &grad_lse)
{
    return sa_backward(volumes, sa_place(volumes, &coords, nullptr, nullptr, {}, {}), beta, lse, moment, grad_kp, grad_lse);
}

at::Tensor soft_argmax3d_cuboid_backward_native(const at::Tensor &volumes, const at::Tensor &rot, const at::Tensor &center, at::ArrayRef<double> position,
                                                at::ArrayRef<double> sides, double beta, const at::Tensor &lse, const at::Tensor &moment,
                                                const c10::optional<at::Tensor> &grad_kp, const c10::optional<at::Tensor> &grad_lse)
{
    return sa_backward(volumes, sa_place(volumes, nullptr, &rot, &center, position, sides), beta, lse, moment, grad_kp, grad_lse);
}

// grad_coords (B,X,Y,Z,3) of the tensor route
at::Tensor soft_argmax3d_backward_coords_native(const at::Tensor &volumes, double beta, const at::Tensor &lse, const at::Tensor &grad_kp)
{
    sa_check_volumes(volumes);
    const int64_t B = volumes.size(0), J = volumes.size(1), X = volumes.size(2), Y = volumes.size(3), Z = volumes.size(4);
    check_tensor(lse, volumes, "logsumexp (B, J)", at::kFloat, B * J);
    check_tensor(grad_kp, volumes, "grad_keypoints (B, J, 3)", at::kFloat, B * J * 3);
    c10::DeviceGuard guard(volumes.device());
    at::Tensor gc = at::empty({B, X, Y, Z, 3}, volumes.options().dtype(at::kFloat));
    check_status(mvhmr_soft_argmax3d_backward_coords(volumes.data_ptr(), sa_dtype(volumes), (int32_t)B, (int32_t)J, (int32_t)X, (int32_t)Y, (int32_t)Z, beta,
                                                     lse.data_ptr<float>(), grad_kp.data_ptr<float>(), gc.data_ptr<float>(),
                                                     c10::hip::getCurrentHIPStream(volumes.device().index()).stream()));
    return gc;
}

// grad_rot (B,3,3) and grad_center (B,3) of the cuboid route
std::tuple<at::Tensor, at::Tensor> soft_argmax3d_backward_pose_native(const at::Tensor &rot, const at::Tensor &moment, const at::Tensor &grad_kp)
{
    TORCH_CHECK(rot.is_cuda() && rot.dim() == 3 && rot.size(1) == 3 && rot.size(2) == 3 && moment.dim() == 3 && moment.size(0) == rot.size(0) &&
                moment.size(1) >= 1 && moment.size(2) == 3, "mvhmr_soft_argmax3d: rotations must be (B, 3, 3) on a HIP device and moment (B, J, 3)");
    const int64_t B = rot.size(0), J = moment.size(1);
    TORCH_CHECK(B >= 1 && B * J < (int64_t(1) << 31), "mvhmr_soft_argmax3d: B*J must stay below 2^31");
    check_tensor(rot, rot, "rotations (B, 3, 3)", at::kFloat, B * 9);
    check_tensor(moment, rot, "moment (B, J, 3)", at::kFloat, B * J * 3);
    check_tensor(grad_kp, rot, "grad_keypoints (B, J, 3)", at::kFloat, B * J * 3);
    c10::DeviceGuard guard(rot.device());
    at::Tensor gr = at::empty({B, 3, 3}, rot.options()), gc = at::empty({B, 3}, rot.options());
    check_status(mvhmr_soft_argmax3d_backward_pose(rot.data_ptr<float>(), moment.data_ptr<float>(), grad_kp.data_ptr<float>(), gr.data_ptr<float>(),
                                                   gc.data_ptr<float>(), (int32_t)B, (int32_t)J, c10::hip::getCurrentHIPStream(rot.device().index()).stream()));
    return {gr, gc};
}


// Trilinear volume sampling at world points (mvhmr_sample_volume_*; multiviewhmr_amd/volsample.py): volumes (B,C,X,Y,Z) fp32 / fp16 / bf16 on
// the cuboid of rot (B,3,3), center (B,3), position, sides; points (B,N,3); every tensor but the volume fp32.  The same per-call tail again.
struct VsCall {
    int64_t B, C, X, Y, Z, N;
    int32_t dtype, paired;
    hipStream_t stream;
};

VsCall vs_open(const at::Tensor &volumes, int64_t points, bool paired)
{
    TORCH_CHECK(volumes.is_cuda() && volumes.is_contiguous() && volumes.dim() == 5 && volumes.numel() > 0,
                "mvhmr_sample_volume: volumes must be a contiguous, non-empty (B, C, X, Y, Z) tensor on a HIP device");
    VsCall c{volumes.size(0), volumes.size(1), volumes.size(2), volumes.size(3), volumes.size(4), points, 0, paired ? 1 : 0, nullptr};
    TORCH_CHECK(c.X >= 2 && c.Y >= 2 && c.Z >= 2, "mvhmr_sample_volume: every extent of the volume must be >= 2");
    const int64_t lim = int64_t(1) << 31;
    TORCH_CHECK(c.N >= 1 && c.X * c.Y * c.Z < lim && c.B * c.C < lim && c.B * c.N < lim, "mvhmr_sample_volume: N >= 1; X*Y*Z, B*C and B*N must stay below 2^31");
    TORCH_CHECK(!paired || c.N == c.C, "mvhmr_sample_volume: a paired call needs N == C, got N = ", c.N, ", C = ", c.C);
    c.dtype = sa_dtype(volumes);
    c.stream = c10::hip::getCurrentHIPStream(volumes.device().index()).stream();
    return c;
}

void vs_check_place(const VsCall &c, const at::Tensor &volumes, const at::Tensor &points, const at::Tensor &rot, const at::Tensor &center,
                    at::ArrayRef<double> position, at::ArrayRef<double> sides)
{
    TORCH_CHECK(position.size() == 3 && sides.size() == 3, "mvhmr_sample_volume: position and sides take 3 values each");
    TORCH_CHECK(points.dim() == 3 && points.size(0) == c.B && points.size(2) == 3, "mvhmr_sample_volume: points must be (B, N, 3)");
    check_tensor(points, volumes, "points (B, N, 3)", at::kFloat, c.B * c.N * 3);
    check_tensor(rot, volumes, "rotations (B, 3, 3)", at::kFloat, c.B * 9);
    check_tensor(center, volumes, "centers (B, 3)", at::kFloat, c.B * 3);
}

int64_t vs_sample_numel(const VsCall &c) { return c.paired ? c.B * c.C : c.B * c.C * c.N; }

at::Tensor vs_workspace(const VsCall &c, const at::Tensor &volumes, size_t *bytes)
{
    *bytes = mvhmr_sample_volume_workspace_bytes((int32_t)c.B, (int32_t)c.N);
    return at::empty({(int64_t)*bytes}, volumes.options().dtype(at::kByte));
}

std::tuple<at::Tensor, at::Tensor> sample_volume_native(const at::Tensor &volumes, const at::Tensor &points, const at::Tensor &rot, const at::Tensor &center,
                                                        at::ArrayRef<double> position, at::ArrayRef<double> sides, bool paired)
{
    const VsCall c = vs_open(volumes, points.dim() == 3 ? points.size(1) : 0, paired);
    vs_check_place(c, volumes, points, rot, center, position, sides);
    c10::DeviceGuard guard(volumes.device());
    const auto f32 = volumes.options().dtype(at::kFloat);
    at::Tensor samples = paired ? at::empty({c.B, c.C}, f32) : at::empty({c.B, c.C, c.N}, f32), index = at::empty({c.B, c.N, 3}, f32);
    check_status(mvhmr_sample_volume_forward(volumes.data_ptr(), c.dtype, points.data_ptr<float>(), rot.data_ptr<float>(), center.data_ptr<float>(),
                                             position.data(), sides.data(), (int32_t)c.B, (int32_t)c.C, (int32_t)c.X, (int32_t)c.Y, (int32_t)c.Z, (int32_t)c.N,
                                             c.paired, samples.data_ptr<float>(), index.data_ptr<float>(), c.stream));
    return {samples, index};
}

// grad_volumes, shaped and typed like volumes (of which only shape, dtype and device are read)
at::Tensor sample_volume_backward_volumes_native(const at::Tensor &volumes, const at::Tensor &index, const at::Tensor &grad_samples, bool paired)
{
    const VsCall c = vs_open(volumes, index.dim() == 3 ? index.size(1) : 0, paired);
    check_tensor(index, volumes, "index (B, N, 3)", at::kFloat, c.B * c.N * 3);
    check_tensor(grad_samples, volumes, "grad_samples", at::kFloat, vs_sample_numel(c));
    c10::DeviceGuard guard(volumes.device());
    at::Tensor gv = at::empty_like(volumes);
    size_t need;
    at::Tensor ws = vs_workspace(c, volumes, &need);
    check_status(mvhmr_sample_volume_backward_volumes(c.dtype, index.data_ptr<float>(), grad_samples.data_ptr<float>(), (int32_t)c.B, (int32_t)c.C, (int32_t)c.X,
                                                      (int32_t)c.Y, (int32_t)c.Z, (int32_t)c.N, c.paired, gv.data_ptr(), ws.data_ptr(), need, c.stream));
    return gv;
}

// (grad_points (B,N,3), grad_rot (B,3,3), grad_center (B,3)); what is not asked for comes back with 0 elements
std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_volume_backward_geometry_native(const at::Tensor &volumes, const at::Tensor &points, const at::Tensor &rot,
                                                                                      const at::Tensor &center, at::ArrayRef<double> position,
                                                                                      at::ArrayRef<double> sides, bool paired, const at::Tensor &index,
                                                                                      const at::Tensor &grad_samples, bool need_points, bool need_pose)
{
    const VsCall c = vs_open(volumes, points.dim() == 3 ? points.size(1) : 0, paired);
    vs_check_place(c, volumes, points, rot, center, position, sides);
    check_tensor(index, volumes, "index (B, N, 3)", at::kFloat, c.B * c.N * 3);
    check_tensor(grad_samples, volumes, "grad_samples", at::kFloat, vs_sample_numel(c));
    TORCH_CHECK(need_points || need_pose, "mvhmr_sample_volume: the geometry backward needs an output to compute");
    c10::DeviceGuard guard(volumes.device());
    const auto f32 = volumes.options().dtype(at::kFloat);
    at::Tensor gp = at::empty({need_points ? c.B : 0, c.N, 3}, f32), gr = at::empty({need_pose ? c.B : 0, 3, 3}, f32), gc = at::empty({need_pose ? c.B : 0, 3}, f32);
    size_t need;
    at::Tensor ws = vs_workspace(c, volumes, &need);
    check_status(mvhmr_sample_volume_backward_geometry(volumes.data_ptr(), c.dtype, points.data_ptr<float>(), rot.data_ptr<float>(), center.data_ptr<float>(),
                                                       position.data(), sides.data(), (int32_t)c.B, (int32_t)c.C, (int32_t)c.X, (int32_t)c.Y, (int32_t)c.Z,
                                                       (int32_t)c.N, c.paired, index.data_ptr<float>(), grad_samples.data_ptr<float>(),
                                                       need_points ? gp.data_ptr<float>() : nullptr, need_pose ? gr.data_ptr<float>() : nullptr,
                                                       need_pose ? gc.data_ptr<float>() : nullptr, ws.data_ptr(), need, c.stream));
    return {gp, gr, gc};
}


// Ray-marching volumes into camera-view maps (mvhmr_project_volume_*; multiviewhmr_amd/volproject.py): volumes (B,C,X,Y,Z) fp32 / fp16 / bf16 on
// the cuboid of rot (B,3,3), center (B,3), position, sides; rays (B,V,3,4) fp32.  maps (B,V,C,Hm,Wm) and ranges (B,V,Hm,Wm,2) fp32; aux is what
// the backward reads besides: the arg-k (int32, max), the log-sum-exp (fp32, softmax), nothing (0 elements, mean).
struct PvCall {
    int64_t B, C, X, Y, Z, V, Hm, Wm, K;
    int32_t dtype, method;
    hipStream_t stream;
};

PvCall pv_open(const at::Tensor &volumes, const at::Tensor &rays, const at::Tensor &rot, const at::Tensor &center, at::ArrayRef<double> position,
               at::ArrayRef<double> sides, int64_t map_h, int64_t map_w, int64_t n_samples, int64_t method)
{
    TORCH_CHECK(volumes.is_cuda() && volumes.is_contiguous() && volumes.dim() == 5 && volumes.numel() > 0,
                "mvhmr_project_volume: volumes must be a contiguous, non-empty (B, C, X, Y, Z) tensor on a HIP device");
    TORCH_CHECK(rays.dim() == 4 && rays.size(0) == volumes.size(0) && rays.size(1) >= 1 && rays.size(2) == 3 && rays.size(3) == 4,
                "mvhmr_project_volume: rays must be (B, V, 3, 4)");
    PvCall c{volumes.size(0), volumes.size(1), volumes.size(2), volumes.size(3), volumes.size(4), rays.size(1), map_h, map_w, n_samples, 0, (int32_t)method, nullptr};
    TORCH_CHECK(c.X >= 2 && c.Y >= 2 && c.Z >= 2, "mvhmr_project_volume: every extent of the volume must be >= 2");
    TORCH_CHECK(c.Hm >= 1 && c.Wm >= 1 && c.K >= 1 && c.K <= mvhmr_project_volume_max_samples(), "mvhmr_project_volume: map extents >= 1, 1 <= n_samples <= ",
                mvhmr_project_volume_max_samples());
    const int64_t lim = int64_t(1) << 31;
    TORCH_CHECK(c.X * c.Y * c.Z < lim && c.B * c.C * c.V < lim && c.Hm * c.Wm < lim && c.V * c.Hm * c.Wm < lim && c.V * c.Hm * c.Wm * c.K < lim,
                "mvhmr_project_volume: X*Y*Z, B*C*V and V*Hm*Wm*n_samples must stay below 2^31");
    TORCH_CHECK(position.size() == 3 && sides.size() == 3, "mvhmr_project_volume: position and sides take 3 values each");
    check_tensor(rays, volumes, "rays (B, V, 3, 4)", at::kFloat, c.B * c.V * 12);
    check_tensor(rot, volumes, "rotations (B, 3, 3)", at::kFloat, c.B * 9);
    check_tensor(center, volumes, "centers (B, 3)", at::kFloat, c.B * 3);
    c.dtype = sa_dtype(volumes);
    c.stream = c10::hip::getCurrentHIPStream(volumes.device().index()).stream();
    return c;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> project_volume_native(const at::Tensor &volumes, const at::Tensor &rays, const at::Tensor &rot,
                                                                     const at::Tensor &center, at::ArrayRef<double> position, at::ArrayRef<double> sides,
                                                                     int64_t map_h, int64_t map_w, int64_t n_samples, int64_t method, double beta,
                                                                     double min_depth, double max_depth)
{
    const PvCall c = pv_open(volumes, rays, rot, center, position, sides, map_h, map_w, n_samples, method);
    c10::DeviceGuard guard(volumes.device());
    const auto f32 = volumes.options().dtype(at::kFloat);
    at::Tensor maps = at::empty({c.B, c.V, c.C, c.Hm, c.Wm}, f32), ranges = at::empty({c.B, c.V, c.Hm, c.Wm, 2}, f32);
    at::Tensor aux = method == MVHMR_PROJECT_MAX       ? at::empty({c.B, c.V, c.C, c.Hm, c.Wm}, f32.dtype(at::kInt))
                     : method == MVHMR_PROJECT_SOFTMAX ? at::empty({c.B, c.V, c.C, c.Hm, c.Wm}, f32)
                                                       : at::empty({0}, f32);
    check_status(mvhmr_project_volume_forward(volumes.data_ptr(), c.dtype, rays.data_ptr<float>(), rot.data_ptr<float>(), center.data_ptr<float>(),
                                              position.data(), sides.data(), (int32_t)c.B, (int32_t)c.V, (int32_t)c.C, (int32_t)c.X, (int32_t)c.Y, (int32_t)c.Z,
                                              (int32_t)c.Hm, (int32_t)c.Wm, (int32_t)c.K, c.method, beta, min_depth, max_depth, maps.data_ptr<float>(),
                                              ranges.data_ptr<float>(), aux.numel() ? aux.data_ptr() : nullptr, c.stream));
    return {maps, ranges, aux};
}

// grad_volumes, shaped and typed like volumes; the workspace (the int64 accumulator of one pass of channels) comes from torch's allocator
at::Tensor project_volume_backward_volumes_native(const at::Tensor &volumes, const at::Tensor &rays, const at::Tensor &rot, const at::Tensor &center,
                                                  at::ArrayRef<double> position, at::ArrayRef<double> sides, int64_t map_h, int64_t map_w, int64_t n_samples,
                                                  int64_t method, double beta, double min_depth, double max_depth, const at::Tensor &grad_maps,
                                                  const at::Tensor &maps, const at::Tensor &aux)
{
    const PvCall c = pv_open(volumes, rays, rot, center, position, sides, map_h, map_w, n_samples, method);
    const int64_t n = c.B * c.V * c.C * c.Hm * c.Wm;
    check_tensor(grad_maps, volumes, "grad_maps (B, V, C, Hm, Wm)", at::kFloat, n);
    check_tensor(maps, volumes, "maps (B, V, C, Hm, Wm)", at::kFloat, n);
    if (method == MVHMR_PROJECT_MAX) check_tensor(aux, volumes, "aux (B, V, C, Hm, Wm)", at::kInt, n);
    if (method == MVHMR_PROJECT_SOFTMAX) check_tensor(aux, volumes, "aux (B, V, C, Hm, Wm)", at::kFloat, n);
    c10::DeviceGuard guard(volumes.device());
    at::Tensor gv = at::empty_like(volumes);
    const size_t need = mvhmr_project_volume_workspace_bytes((int32_t)c.B, (int32_t)c.C, (int32_t)c.X, (int32_t)c.Y, (int32_t)c.Z);
    at::Tensor ws = at::empty({(int64_t)need}, volumes.options().dtype(at::kByte));
    check_status(mvhmr_project_volume_backward_volumes(volumes.data_ptr(), c.dtype, rays.data_ptr<float>(), rot.data_ptr<float>(), center.data_ptr<float>(),
                                                       position.data(), sides.data(), (int32_t)c.B, (int32_t)c.V, (int32_t)c.C, (int32_t)c.X, (int32_t)c.Y,
                                                       (int32_t)c.Z, (int32_t)c.Hm, (int32_t)c.Wm, (int32_t)c.K, c.method, beta, min_depth, max_depth,
                                                       grad_maps.data_ptr<float>(), maps.data_ptr<float>(), aux.numel() ? aux.data_ptr() : nullptr,
                                                       gv.data_ptr(), ws.data_ptr(), need, c.stream));
    return gv;
}


// 3-D non-maximum suppression and top-K proposals (mvhmr_volume_peaks*; multiviewhmr_amd/peaks.py): volumes (B,J,X,Y,Z) fp32 / fp16 / bf16 in,
// scores (B,J,K) fp32 and index (B,J,K) int32 out, and with a cuboid (rot != null) positions (B,J,K,3) fp32.
int32_t pk_dtype(at::ScalarType t)
{
    TORCH_CHECK(t == at::kFloat || t == at::kHalf || t == at::kBFloat16, "mvhmr_volume_peaks: volumes must be fp32, fp16 or bf16, got ", t);
    return t == at::kHalf ? MVHMR_F16 : t == at::kBFloat16 ? MVHMR_BF16 : MVHMR_F32;
}

void pk_check_sizes(at::IntArrayRef shape, int64_t k)
{
    TORCH_CHECK(shape.size() == 5, "mvhmr_volume_peaks: volumes must be (B, J, X, Y, Z)");
    for (int64_t e : shape) TORCH_CHECK(e >= 1, "mvhmr_volume_peaks: volumes must not be empty");
    const int64_t lim = int64_t(1) << 31;
    for (int64_t e : shape) TORCH_CHECK(e < lim, "mvhmr_volume_peaks: every extent must stay below 2^31");                 // so that no product below overflows
    TORCH_CHECK(shape[2] * shape[3] < lim && shape[2] * shape[3] * shape[4] < lim && shape[0] * shape[1] < lim,
                "mvhmr_volume_peaks: X*Y*Z and B*J must stay below 2^31");
    TORCH_CHECK(k >= 1 && k <= mvhmr_volume_peaks_max_k(), "mvhmr_volume_peaks: k must be 1 .. ", mvhmr_volume_peaks_max_k(), ", got ", k);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> pk_forward(const at::Tensor &volumes, const at::Tensor *rot, const at::Tensor *center,
                                                          at::ArrayRef<double> position, at::ArrayRef<double> sides, int64_t k, int64_t radius,
                                                          double threshold)
{
    TORCH_CHECK(volumes.is_cuda() && volumes.is_contiguous() && volumes.dim() == 5,
                "mvhmr_volume_peaks: volumes must be a contiguous (B, J, X, Y, Z) tensor on a HIP device");
    pk_check_sizes(volumes.sizes(), k);
    TORCH_CHECK(radius >= 0 && radius <= 3, "mvhmr_volume_peaks: radius must be 0 .. 3, got ", radius);
    TORCH_CHECK(threshold == threshold, "mvhmr_volume_peaks: threshold must not be NaN");
    const int32_t dtype = pk_dtype(volumes.scalar_type());
    const int64_t B = volumes.size(0), J = volumes.size(1), X = volumes.size(2), Y = volumes.size(3), Z = volumes.size(4);
    if (rot) {
        TORCH_CHECK(position.size() == 3 && sides.size() == 3, "mvhmr_volume_peaks: position and sides take 3 values each");
        check_tensor(*rot, volumes, "rotations (B, 3, 3)", at::kFloat, B * 9);
        check_tensor(*center, volumes, "centers (B, 3)", at::kFloat, B * 3);
    }
    c10::DeviceGuard guard(volumes.device());
    const auto f32 = volumes.options().dtype(at::kFloat);
    at::Tensor scores = at::empty({B, J, k}, f32), index = at::empty({B, J, k}, volumes.options().dtype(at::kInt));
    at::Tensor positions = rot ? at::empty({B, J, k, 3}, f32) : at::Tensor();
    const size_t need = mvhmr_volume_peaks_workspace_bytes((int32_t)B, (int32_t)J, (int32_t)X, (int32_t)Y, (int32_t)Z, (int32_t)k);
    at::Tensor ws = at::empty({(int64_t)need}, volumes.options().dtype(at::kByte));
    check_status(mvhmr_volume_peaks(volumes.data_ptr(), dtype, (int32_t)B, (int32_t)J, (int32_t)X, (int32_t)Y, (int32_t)Z, (int32_t)k, (int32_t)radius,
                                    (float)threshold, rot ? rot->data_ptr<float>() : nullptr, rot ? center->data_ptr<float>() : nullptr,
                                    rot ? position.data() : nullptr, rot ? sides.data() : nullptr, scores.data_ptr<float>(), index.data_ptr<int32_t>(),
                                    rot ? positions.data_ptr<float>() : nullptr, ws.data_ptr(), need,
                                    c10::hip::getCurrentHIPStream(volumes.device().index()).stream()));
    return {scores, index, positions};
}

std::tuple<at::Tensor, at::Tensor> volume_peaks_native(const at::Tensor &volumes, int64_t k, int64_t radius, double threshold)
{
    auto out = pk_forward(volumes, nullptr, nullptr, {}, {}, k, radius, threshold);
    return {std::get<0>(out), std::get<1>(out)};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> volume_peaks_cuboid_native(const at::Tensor &volumes, const at::Tensor &rot, const at::Tensor &center,
                                                                          at::ArrayRef<double> position, at::ArrayRef<double> sides, int64_t k,
                                                                          int64_t radius, double threshold)
{
    return pk_forward(volumes, &rot, &center, position, sides, k, radius, threshold);
}

// grad_volumes of `shape` and `dtype` from index and grad_scores (B, J, K): the volume itself is not needed
at::Tensor volume_peaks_backward_native(const at::Tensor &index, const at::Tensor &grad_scores, at::IntArrayRef shape, at::ScalarType dtype)
{
    TORCH_CHECK(index.is_cuda() && index.is_contiguous() && index.dim() == 3 && index.scalar_type() == at::kInt,
                "mvhmr_volume_peaks: index must be a contiguous (B, J, K) int32 tensor on a HIP device");
    pk_check_sizes(shape, index.size(2));
    TORCH_CHECK(index.size(0) == shape[0] && index.size(1) == shape[1], "mvhmr_volume_peaks: index must be (B, J, K) of the volumes' B and J");
    check_tensor(grad_scores, index, "grad_scores (B, J, K)", at::kFloat, index.numel());
    const int32_t dt = pk_dtype(dtype);
    c10::DeviceGuard guard(index.device());
    at::Tensor gv = at::empty(shape, index.options().dtype(dtype));
    check_status(mvhmr_volume_peaks_backward(dt, index.data_ptr<int32_t>(), grad_scores.data_ptr<float>(), (int32_t)shape[0], (int32_t)shape[1],
                                             (int32_t)shape[2], (int32_t)shape[3], (int32_t)shape[4], (int32_t)index.size(2), gv.data_ptr(),
                                             c10::hip::getCurrentHIPStream(index.device().index()).stream()));
    return gv;
}

// (grad_rot (B,3,3), grad_center (B,3)) from index and grad_positions (B, J, K, 3); vol is (X, Y, Z)
std::tuple<at::Tensor, at::Tensor> volume_peaks_backward_pose_native(const at::Tensor &index, const at::Tensor &grad_positions, const at::Tensor &rot,
                                                                     const at::Tensor &center, at::ArrayRef<double> position, at::ArrayRef<double> sides,
                                                                     at::IntArrayRef vol)
{
    TORCH_CHECK(index.is_cuda() && index.is_contiguous() && index.dim() == 3 && index.scalar_type() == at::kInt,
                "mvhmr_volume_peaks: index must be a contiguous (B, J, K) int32 tensor on a HIP device");
    TORCH_CHECK(vol.size() == 3 && position.size() == 3 && sides.size() == 3, "mvhmr_volume_peaks: vol, position and sides take 3 values each");
    const int64_t B = index.size(0), J = index.size(1), K = index.size(2);
    pk_check_sizes({B, J, vol[0], vol[1], vol[2]}, K);
    check_tensor(grad_positions, index, "grad_positions (B, J, K, 3)", at::kFloat, index.numel() * 3);
    check_tensor(rot, index, "rotations (B, 3, 3)", at::kFloat, B * 9);
    check_tensor(center, index, "centers (B, 3)", at::kFloat, B * 3);
    c10::DeviceGuard guard(index.device());
    const auto f32 = index.options().dtype(at::kFloat);
    at::Tensor gr = at::empty({B, 3, 3}, f32), gc = at::empty({B, 3}, f32);
    check_status(mvhmr_volume_peaks_backward_pose(index.data_ptr<int32_t>(), grad_positions.data_ptr<float>(), rot.data_ptr<float>(), center.data_ptr<float>(),
                                                  position.data(), sides.data(), (int32_t)B, (int32_t)J, (int32_t)vol[0], (int32_t)vol[1], (int32_t)vol[2],
                                                  (int32_t)K, gr.data_ptr<float>(), gc.data_ptr<float>(),
                                                  c10::hip::getCurrentHIPStream(index.device().index()).stream()));
    return {gr, gc};
}

}  // namespace

// the descriptor's fields after an op's tensors, and the cuboid ops' arguments
#define MVHMR_DESC_ARGS "int B, int V, int C, int H, int W, int method, int feat_dtype, int out_dtype, int layout, int variant"
#define MVHMR_CUBOID_ARGS "Tensor proj, Tensor rot, Tensor center, float[] position, float[] sides, int[] vol, " MVHMR_DESC_ARGS
#define MVHMR_MASK_ARG ", Tensor? view_mask=None"
#define MVHMR_WEIGHTS_ARG ", Tensor? view_weights=None"
#define MVHMR_GRAD_WEIGHTS_ARG ", Tensor(a!)? grad_weights=None"
#define MVHMR_VISIBLE_ARG ", bool visible_only=False"
#define MVHMR_CONF_ARG ", Tensor? view_confidence=None"
#define MVHMR_GRAD_CONF_ARG ", Tensor(b!)? grad_confidence=None"
#define MVHMR_INDEX_ARG ", int moments=0, Tensor? feature_index=None, Tensor? lens=None"      // (moments: the cross-view variance; the index and the lens stay last)

TORCH_LIBRARY(mvhmr_native, m)
{
    m.def("unprojection(Tensor features, Tensor proj, Tensor coords, " MVHMR_DESC_ARGS MVHMR_MASK_ARG MVHMR_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_INDEX_ARG ") -> Tensor");
    m.def("unprojection_backward(Tensor grad_out, Tensor features, Tensor proj, Tensor coords, " MVHMR_DESC_ARGS MVHMR_MASK_ARG
          ", bool deterministic=False" MVHMR_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_INDEX_ARG ") -> Tensor");
    m.def("unprojection_backward_geometry(Tensor grad_out, Tensor features, Tensor proj, Tensor coords, " MVHMR_DESC_ARGS
          ", bool want_proj, bool want_coords" MVHMR_MASK_ARG MVHMR_WEIGHTS_ARG MVHMR_GRAD_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_GRAD_CONF_ARG MVHMR_INDEX_ARG ") -> (Tensor, Tensor)");
    m.def("unprojection_cuboid(Tensor features, " MVHMR_CUBOID_ARGS MVHMR_MASK_ARG MVHMR_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_INDEX_ARG ") -> Tensor");
    m.def("unprojection_cuboid_backward(Tensor grad_out, Tensor features, " MVHMR_CUBOID_ARGS MVHMR_MASK_ARG ", bool deterministic=False" MVHMR_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_INDEX_ARG ") -> Tensor");
    m.def("unprojection_cuboid_backward_geometry(Tensor grad_out, Tensor features, " MVHMR_CUBOID_ARGS
          ", bool want_proj, bool want_rot, bool want_center" MVHMR_MASK_ARG MVHMR_WEIGHTS_ARG MVHMR_GRAD_WEIGHTS_ARG MVHMR_VISIBLE_ARG MVHMR_CONF_ARG MVHMR_GRAD_CONF_ARG MVHMR_INDEX_ARG ") -> (Tensor, Tensor, Tensor)");
    m.def("triangulate_dlt(Tensor proj, Tensor points, Tensor? confidences) -> Tensor");
    m.def("triangulate_dlt_backward(Tensor grad_out, Tensor proj, Tensor points, Tensor? confidences) -> (Tensor, Tensor, Tensor)");
    m.def("abi_version() -> int");
}

TORCH_LIBRARY_IMPL(mvhmr_native, CUDA, m)
{
    m.impl("unprojection", &unprojection_native);
    m.impl("unprojection_backward", &unprojection_backward_native);
    m.impl("unprojection_backward_geometry", &unprojection_backward_geometry_native);
    m.impl("unprojection_cuboid", &unprojection_cuboid_native);
    m.impl("unprojection_cuboid_backward", &unprojection_cuboid_backward_native);
    m.impl("unprojection_cuboid_backward_geometry", &unprojection_cuboid_backward_geometry_native);
    m.impl("triangulate_dlt", &triangulate_dlt_native);
    m.impl("triangulate_dlt_backward", &triangulate_dlt_backward_native);
}

// the visibility bits are no un-projection: a namespace of their own, mvhmr_native holds the six un-projection ops and the DLT
TORCH_LIBRARY(mvhmr_visibility, m)
{
    m.def("view_visibility(Tensor proj, Tensor coords, int H, int W, Tensor? view_mask=None) -> Tensor");
    m.def("view_visibility_cuboid(Tensor proj, Tensor rot, Tensor center, float[] position, float[] sides, int[] vol, int H, int W, Tensor? view_mask=None) -> Tensor");
}

TORCH_LIBRARY_IMPL(mvhmr_visibility, CUDA, m)
{
    m.impl("view_visibility", &view_visibility_native);
    m.impl("view_visibility_cuboid", &view_visibility_cuboid_native);
}

// the volumetric soft-argmax reads a volume, it un-projects nothing: a namespace of its own as well
TORCH_LIBRARY(mvhmr_softargmax, m)
{
    m.def("soft_argmax3d(Tensor volumes, Tensor coords, float beta) -> (Tensor, Tensor, Tensor)");
    m.def("soft_argmax3d_cuboid(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, float beta) -> (Tensor, Tensor, Tensor)");
    m.def("soft_argmax3d_backward(Tensor volumes, Tensor coords, float beta, Tensor logsumexp, Tensor moment, Tensor? grad_keypoints, Tensor? grad_logsumexp) -> Tensor");
    m.def("soft_argmax3d_cuboid_backward(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, float beta, Tensor logsumexp, Tensor moment, "
          "Tensor? grad_keypoints, Tensor? grad_logsumexp) -> Tensor");
    m.def("soft_argmax3d_backward_coords(Tensor volumes, float beta, Tensor logsumexp, Tensor grad_keypoints) -> Tensor");
    m.def("soft_argmax3d_backward_pose(Tensor rot, Tensor moment, Tensor grad_keypoints) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(mvhmr_softargmax, CUDA, m)
{
    m.impl("soft_argmax3d", &soft_argmax3d_native);
    m.impl("soft_argmax3d_cuboid", &soft_argmax3d_cuboid_native);
    m.impl("soft_argmax3d_backward", &soft_argmax3d_backward_native);
    m.impl("soft_argmax3d_cuboid_backward", &soft_argmax3d_cuboid_backward_native);
    m.impl("soft_argmax3d_backward_coords", &soft_argmax3d_backward_coords_native);
    m.impl("soft_argmax3d_backward_pose", &soft_argmax3d_backward_pose_native);
}

// reading a volume back at world points: again neither un-projection nor soft-argmax
TORCH_LIBRARY(mvhmr_volsample, m)
{
    m.def("sample_volume(Tensor volumes, Tensor points, Tensor rot, Tensor center, float[] position, float[] sides, bool paired) -> (Tensor, Tensor)");
    m.def("sample_volume_backward_volumes(Tensor volumes, Tensor index, Tensor grad_samples, bool paired) -> Tensor");
    m.def("sample_volume_backward_geometry(Tensor volumes, Tensor points, Tensor rot, Tensor center, float[] position, float[] sides, bool paired, "
          "Tensor index, Tensor grad_samples, bool need_points, bool need_pose) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(mvhmr_volsample, CUDA, m)
{
    m.impl("sample_volume", &sample_volume_native);
    m.impl("sample_volume_backward_volumes", &sample_volume_backward_volumes_native);
    m.impl("sample_volume_backward_geometry", &sample_volume_backward_geometry_native);
}

// peaks of a heat volume: a reader of volumes like the two above, with integer outputs
TORCH_LIBRARY(mvhmr_peaks, m)
{
    m.def("volume_peaks(Tensor volumes, int k, int radius, float threshold) -> (Tensor, Tensor)");
    m.def("volume_peaks_cuboid(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, int k, int radius, float threshold) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("volume_peaks_backward(Tensor index, Tensor grad_scores, int[] shape, ScalarType dtype) -> Tensor");
    m.def("volume_peaks_backward_pose(Tensor index, Tensor grad_positions, Tensor rot, Tensor center, float[] position, float[] sides, int[] vol) -> "
          "(Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(mvhmr_peaks, CUDA, m)
{
    m.impl("volume_peaks", &volume_peaks_native);
    m.impl("volume_peaks_cuboid", &volume_peaks_cuboid_native);
    m.impl("volume_peaks_backward", &volume_peaks_backward_native);
    m.impl("volume_peaks_backward_pose", &volume_peaks_backward_pose_native);
}

// rendering a volume into the cameras: a reader of volumes and of rays, the fourth of its kind
TORCH_LIBRARY(mvhmr_volproject, m)
{
    m.def("project_volume(Tensor volumes, Tensor rays, Tensor rot, Tensor center, float[] position, float[] sides, int map_h, int map_w, int n_samples, "
          "int method, float beta, float min_depth, float max_depth) -> (Tensor, Tensor, Tensor)");
    m.def("project_volume_backward_volumes(Tensor volumes, Tensor rays, Tensor rot, Tensor center, float[] position, float[] sides, int map_h, int map_w, "
          "int n_samples, int method, float beta, float min_depth, float max_depth, Tensor grad_maps, Tensor maps, Tensor aux) -> Tensor");
}

TORCH_LIBRARY_IMPL(mvhmr_volproject, CUDA, m)
{
    m.impl("project_volume", &project_volume_native);
    m.impl("project_volume_backward_volumes", &project_volume_backward_volumes_native);
}

TORCH_LIBRARY_IMPL(mvhmr_native, CompositeExplicitAutograd, m)
{
    m.impl("abi_version", []() -> int64_t { return mvhmr_abi_version(); });
}
