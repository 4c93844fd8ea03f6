// Counter-based decoder noise: the 13 noise planes of a SynthesisNetwork pass (styleganv1.py:448-456: ApplyNoise draws
// torch.randn inside forward) as ONE launch whose every value is a pure function of (seed, frame, layer, pixel) -- the
// definition in include/spk.h.  No generator state is read or advanced, so a clip renders the same frames whatever the chunking
// or the sharding over devices, and a fixed-noise clip (every frame on one frame index) needs no expanded tensors.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): one block = four 32-bit
// words = four pixels; integer multiplies, xors and adds only.  The block function is one __host__ __device__ routine: the host
// entry point spk_noise_bits_host runs the code the kernel compiles.
#include "spk_common.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int GRID_CAP = 2048;      // workgroups per launch; the rest of the work is a grid-stride trip
constexpr int THREADS = 256;

struct Bits4 { uint32_t v[4]; };

__host__ __device__ inline Bits4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Bits4{{c0, c1, c2, c3}};
}

// the block of (seed, frame, layer, q): ctr = (q, frame lo, layer, frame hi), key = (seed lo, seed hi)
__host__ __device__ inline Bits4 noise_bits(uint64_t seed, int64_t frame, int32_t layer, uint32_t q) {
    const uint64_t f = (uint64_t)frame;
    return philox4x32_10(q, (uint32_t)f, (uint32_t)layer, (uint32_t)(f >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// per launch: where each layer's work items (one Philox block each) and floats start
struct Layout {
    long long item0[SPK_NOISE_MAX_LAYERS + 1];   // first work item of layer l; [n_layers] = the total
    long long off[SPK_NOISE_MAX_LAYERS];         // first float of layer l in dst
    long long hw[SPK_NOISE_MAX_LAYERS];
    int n_layers, layer0;
};

// where batch row b takes its (seed, frame) from: one pair per launch and a step (spk_noise_fill), or two device tables
// (spk_noise_fill_rows)
struct Stepped {
    unsigned long long seed_;
    long long frame0;
    int frame_step;
    __device__ __forceinline__ uint64_t seed(long long) const { return seed_; }
    __device__ __forceinline__ int64_t frame(long long b) const { return frame0 + b * frame_step; }
};
struct Tabled {
    const uint64_t* seeds;
    const int64_t* frames;
    __device__ __forceinline__ uint64_t seed(long long b) const { return seeds[b]; }
    __device__ __forceinline__ int64_t frame(long long b) const { return frames[b]; }
};

// u = ((bits >> 9) + 0.5) * 2^-23: 23 bits + a half, exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float unit_open(uint32_t bits) { return ((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Box-Muller over (u0, u1): the angle 2 pi u1 is taken as sincospi(2 u1) -- 2 u1 is exact, so no rounding of the argument
__device__ __forceinline__ void box_muller(uint32_t b0, uint32_t b1, float& za, float& zb) {
    const float r = sqrtf(-2.f * logf(unit_open(b0)));
    float s, c;
    sincospif(2.f * unit_open(b1), &s, &c);
    za = r * c;
    zb = r * s;
}

// A thread owns one Philox block: four consecutive pixels of one (layer, batch row) plane.  VEC: one float4 store (every plane
// length a multiple of 4 and dst 16-byte aligned, so every block is); else scalar stores with a tail.  Both forms run the same
// arithmetic: the same bits for the same (seed, frame, layer, pixel).  This is the per-block routine of both kernels.
template <bool VEC, class Src>
__device__ __forceinline__ void fill_block(float* __restrict__ dst, const Layout& pl, const Src& src, long long idx) {
    int l = 0;
    while (l + 1 < pl.n_layers && idx >= pl.item0[l + 1]) ++l;
    const long long hw = pl.hw[l], groups = (hw + 3) >> 2;
    const long long r = idx - pl.item0[l];
    long long b;
    if ((unsigned long long)(r | groups) >> 32) b = r / groups;
    else b = (unsigned)r / (unsigned)groups;          // (the decoder's sizes: no 64-bit division)
    const long long q = r - b * groups;
    const Bits4 bits = noise_bits(src.seed(b), src.frame(b), pl.layer0 + l, (uint32_t)q);
    float z[4];
    box_muller(bits.v[0], bits.v[1], z[0], z[1]);
    box_muller(bits.v[2], bits.v[3], z[2], z[3]);
    const long long p0 = q << 2;
    float* out = dst + pl.off[l] + b * hw + p0;
    if (VEC) {
        *reinterpret_cast<float4*>(out) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (p0 + i < hw) out[i] = z[i];
    }
}

template <bool VEC, class Src>
__global__ __launch_bounds__(THREADS) void noise_fill_kernel(float* __restrict__ dst, Layout pl, Src src) {
    const long long total = pl.item0[pl.n_layers];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x)
        fill_block<VEC>(dst, pl, src, idx);
}

// What both entry points check of (dst, B, the layers) and the layout they launch with: -> SPK_OK with `pl`, the float4 rule
// (`vec`), the work items and the floats of dst filled in
int layout(const char* who, const float* dst, int B, int n_layers, int layer0, const int64_t* hws, Layout& pl, bool& vec, long long& items,
           long long& floats) {
    SPK_REQUIRE(dst, "%s: null dst", who);
    SPK_REQUIRE(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    SPK_REQUIRE(n_layers >= 1 && n_layers <= SPK_NOISE_MAX_LAYERS, "%s: n_layers must be in [1, %d] (got %d)", who, SPK_NOISE_MAX_LAYERS,
                n_layers);
    SPK_REQUIRE(layer0 >= 0, "%s: negative layer0 (%d)", who, layer0);
    SPK_REQUIRE(layer0 <= INT32_MAX - SPK_NOISE_MAX_LAYERS, "%s: layer0 + n_layers leaves the 31-bit layer range", who);
    pl = {};
    items = floats = 0;
    vec = (uintptr_t)dst % 16 == 0;
    for (int l = 0; l < n_layers; ++l) {
        const long long hw = hws[l];
        SPK_REQUIRE(hw >= 1, "%s: hw[%d] must be >= 1 (got %lld)", who, l, hw);
        SPK_REQUIRE(hw <= (1ll << 34), "%s: hw[%d] = %lld is more than 2^34 pixels (the block index is 32 bits)", who, l, hw);
        SPK_REQUIRE(hw <= ((1ll << 46) - floats) / B, "%s: more than 2^46 floats up to layer %d", who, l);
        pl.item0[l] = items;
        pl.off[l] = floats;
        pl.hw[l] = hw;
        vec = vec && hw % 4 == 0;
        items += (long long)B * ((hw + 3) >> 2);
        floats += (long long)B * hw;
    }
    pl.item0[n_layers] = items;
    pl.n_layers = n_layers;
    pl.layer0 = layer0;
    return SPK_OK;
}

template <class Src>
int launch(float* dst, const Layout& pl, const Src& src, bool vec, long long items, void* stream) {
    const dim3 grid((unsigned)std::min((items + THREADS - 1) / THREADS, (long long)GRID_CAP));
    if (vec) hipLaunchKernelGGL((noise_fill_kernel<true, Src>), grid, dim3(THREADS), 0, (hipStream_t)stream, dst, pl, src);
    else hipLaunchKernelGGL((noise_fill_kernel<false, Src>), grid, dim3(THREADS), 0, (hipStream_t)stream, dst, pl, src);
    return spk::check_launch("noise_fill_kernel");
}

// [p, p + bytes) and [q, q + qbytes) share a byte
inline bool overlap(const void* p, uint64_t bytes, const void* q, uint64_t qbytes) {
    const uint64_t a = (uint64_t)(uintptr_t)p, b = (uint64_t)(uintptr_t)q;
    return a < b ? b - a < bytes : a - b < qbytes;
}

}  // namespace

extern "C" {

int spk_noise_bits_host(uint64_t seed, int64_t frame, int32_t layer, uint32_t q, uint32_t out[4]) {
    SPK_REQUIRE(out, "noise_bits_host: null output pointer");
    const Bits4 b = noise_bits(seed, frame, layer, q);
    for (int i = 0; i < 4; ++i) out[i] = b.v[i];
    return SPK_OK;
}

int spk_noise_fill(const spk_noise_fill_args* a, void* stream) {
    const char* who = "noise_fill";
    SPK_REQUIRE(a, "%s: null argument struct", who);
    SPK_REQUIRE(a->frame0 >= 0, "%s: negative frame0 (%lld)", who, (long long)a->frame0);
    SPK_REQUIRE(a->frame_step == 0 || a->frame_step == 1, "%s: frame_step must be 0 (fixed) or 1 (fresh) (got %d)", who, a->frame_step);
    Layout pl;
    bool vec;
    long long items, floats;
    if (int rc = layout(who, a->dst, a->B, a->n_layers, a->layer0, a->hw, pl, vec, items, floats)) return rc;
    SPK_REQUIRE(a->frame0 <= INT64_MAX - a->B, "%s: frame0 + B leaves the 63-bit frame range", who);      // (B >= 1 from here on)
    return launch(a->dst, pl, Stepped{a->seed, a->frame0, a->frame_step}, vec, items, stream);
}

int spk_noise_fill_rows(const spk_noise_fill_rows_args* a, void* stream) {
    const char* who = "noise_fill_rows";
    SPK_REQUIRE(a, "%s: null argument struct", who);
    Layout pl;
    bool vec;
    long long items, floats;
    if (int rc = layout(who, a->dst, a->B, a->n_layers, a->layer0, a->hw, pl, vec, items, floats)) return rc;
    SPK_REQUIRE(a->seeds_dev && a->frames_dev, "%s: null seed or frame table", who);
    SPK_REQUIRE((uintptr_t)a->seeds_dev % 8 == 0 && (uintptr_t)a->frames_dev % 8 == 0, "%s: the seed and frame tables must be aligned to 8 bytes",
                who);
    const uint64_t dst_bytes = (uint64_t)floats * sizeof(float), table_bytes = (uint64_t)a->B * 8;
    SPK_REQUIRE(!overlap(a->dst, dst_bytes, a->seeds_dev, table_bytes) && !overlap(a->dst, dst_bytes, a->frames_dev, table_bytes),
                "%s: a table of %d rows overlaps dst", who, a->B);
    return launch(a->dst, pl, Tabled{a->seeds_dev, a->frames_dev}, vec, items, stream);
}

}  // extern "C"
