// Per-sample view masks (include/mvhmr_unproject.h: the *_masked entry points).
//
// A masked call runs the gather / geometry kernels on a packed problem: every sample's present views are moved to view slots
// 0 .. n_b - 1 (in increasing view order), slots n_b .. V - 1 are absent (zero features, zero projections, no part in the aggregate:
// Problem::view_count).  k_view_table builds the slot tables and the packed projections from the mask, one thread per sample;
// k_view_move packs a per-view tensor into slot order (absent slots zero-filled) and unpacks a gradient back into view order
// (masked views zero-filled).  All stream-ordered, no host synchronisation: a masked call stays graph-capturable.
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// [ n_b int (B) | slot -> view int (B,V) | view -> slot int (B,V), -1 when masked | packed proj fp32 (B,V,12) ]
struct TableView {
    int *count, *s2v, *v2s;
    float *proj;
};
__host__ __device__ inline TableView table_view(void *t, int B, int V)
{
    unsigned char *p = static_cast<unsigned char *>(t);
    const size_t a = align256((size_t)B * sizeof(int)), bv = align256((size_t)B * V * sizeof(int));
    return TableView{reinterpret_cast<int *>(p), reinterpret_cast<int *>(p + a), reinterpret_cast<int *>(p + a + bv),
                     reinterpret_cast<float *>(p + a + 2 * bv)};
}

__global__ void __launch_bounds__(64)
k_view_table(const uint8_t *__restrict__ mask, const float *__restrict__ proj, TableView t, int B, int V)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    for (int v = 0; v < V; ++v) {
        const long long bv = (long long)b * V + v;
        if (mask[bv]) {
            const long long bs = (long long)b * V + n;
            t.s2v[bs] = v;
            t.v2s[bv] = n;
            for (int k = 0; k < 12; ++k) t.proj[bs * 12 + k] = proj[bv * 12 + k];
            ++n;
        } else {
            t.v2s[bv] = -1;
        }
    }
    for (int s = n; s < V; ++s) {
        const long long bs = (long long)b * V + s;
        t.s2v[bs] = -1;
        for (int k = 0; k < 12; ++k) t.proj[bs * 12 + k] = 0.f;
    }
    t.count[b] = n;
}

// Per-view confidence weights: a view is present when its mask byte is nonzero (no mask: every view) AND its weight is
// > 0 -- zero, negative and NaN weights mean absent.  The tables and packed projections as k_view_table's, and the weights packed into
// slot order behind them (absent slots 0).
__global__ void __launch_bounds__(64)
k_view_table_weighted(const uint8_t *__restrict__ mask, const float *__restrict__ weights, const float *__restrict__ proj, TableView t,
                      float *__restrict__ packed_w, int B, int V)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    for (int v = 0; v < V; ++v) {
        const long long bv = (long long)b * V + v;
        const float w = weights[bv];
        if ((!mask || mask[bv]) && w > 0.f) {
            const long long bs = (long long)b * V + n;
            t.s2v[bs] = v;
            t.v2s[bv] = n;
            packed_w[bs] = w;
            for (int k = 0; k < 12; ++k) t.proj[bs * 12 + k] = proj[bv * 12 + k];
            ++n;
        } else {
            t.v2s[bv] = -1;
        }
    }
    for (int s = n; s < V; ++s) {
        const long long bs = (long long)b * V + s;
        t.s2v[bs] = -1;
        packed_w[bs] = 0.f;
        for (int k = 0; k < 12; ++k) t.proj[bs * 12 + k] = 0.f;
    }
    t.count[b] = n;
}

// one block row per (sample, slot or view) pair, grid-stride over the T-words of one view.  PACK: dst slot s <- src view s2v[s] (absent
// slots 0); unpack: dst view v <- src slot v2s[v] (masked views 0).  The index is block-uniform: a zero-filled map reads nothing.
template <typename T, bool PACK>
__global__ void __launch_bounds__(256)
k_view_move(const T *__restrict__ src, T *__restrict__ dst, const int *__restrict__ idx, int V, long long words)
{
    const int bv = blockIdx.x, b = bv / V;
    const int from = idx[bv];
    T *d = dst + (long long)bv * words;
    if (from < 0) {
        for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < words; i += (long long)gridDim.y * 256) d[i] = T{};
        return;
    }
    const T *sp = src + ((long long)b * V + from) * words;
    for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < words; i += (long long)gridDim.y * 256) d[i] = sp[i];
}

template <bool PACK>
hipError_t view_move(const void *src, void *dst, const void *table, int B, int V, size_t bytes, hipStream_t s)
{
    const TableView t = table_view(const_cast<void *>(table), B, V);
    const int *idx = PACK ? t.s2v : t.v2s;
    const size_t align = (reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst) | bytes);
    const dim3 block(256);
    auto grid = [&](size_t words) {
        const size_t per = (words + 255) / 256;
        return dim3((unsigned)((size_t)B * V), (unsigned)(per < 64 ? (per ? per : 1) : 64));
    };
    if (align % 16 == 0) {
        hipLaunchKernelGGL((k_view_move<uint4, PACK>), grid(bytes / 16), block, 0, s, (const uint4 *)src, (uint4 *)dst, idx, V, (long long)(bytes / 16));
    } else if (align % 4 == 0) {
        hipLaunchKernelGGL((k_view_move<uint32_t, PACK>), grid(bytes / 4), block, 0, s, (const uint32_t *)src, (uint32_t *)dst, idx, V, (long long)(bytes / 4));
    } else if (align % 2 == 0) {
        hipLaunchKernelGGL((k_view_move<uint16_t, PACK>), grid(bytes / 2), block, 0, s, (const uint16_t *)src, (uint16_t *)dst, idx, V, (long long)(bytes / 2));
    } else {
        hipLaunchKernelGGL((k_view_move<uint8_t, PACK>), grid(bytes), block, 0, s, (const uint8_t *)src, (uint8_t *)dst, idx, V, (long long)bytes);
    }
    return hipGetLastError();
}

}  // namespace

size_t view_table_bytes(int B, int V)
{
    return align256((size_t)B * sizeof(int)) + 2 * align256((size_t)B * V * sizeof(int)) + align256((size_t)B * V * 12 * sizeof(float));
}

hipError_t launch_view_table(const uint8_t *mask, const float *proj, void *table, int B, int V, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_table, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, mask, proj, table_view(table, B, V), B, V);
    return hipGetLastError();
}

// the weighted table: k_view_table's regions, then the packed weights (B, V) fp32
size_t weighted_view_table_bytes(int B, int V) { return view_table_bytes(B, V) + align256((size_t)B * V * sizeof(float)); }
const float *view_table_weights(const void *table, int B, int V)
{
    return reinterpret_cast<const float *>(static_cast<const unsigned char *>(table) + view_table_bytes(B, V));
}

hipError_t launch_view_table_weighted(const uint8_t *mask, const float *weights, const float *proj, void *table, int B, int V, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_table_weighted, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, mask, weights, proj, table_view(table, B, V),
                       const_cast<float *>(view_table_weights(table, B, V)), B, V);
    return hipGetLastError();
}

const int *view_table_counts(const void *table) { return static_cast<const int *>(table); }
const float *view_table_proj(const void *table, int B, int V) { return table_view(const_cast<void *>(table), B, V).proj; }

hipError_t launch_view_pack(const void *src, void *dst, const void *table, int B, int V, size_t bytes_per_view, hipStream_t s)
{
    return view_move<true>(src, dst, table, B, V, bytes_per_view, s);
}

hipError_t launch_view_unpack(const void *src, void *dst, const void *table, int B, int V, size_t bytes_per_view, hipStream_t s)
{
    return view_move<false>(src, dst, table, B, V, bytes_per_view, s);
}

}  // namespace mvhmr
