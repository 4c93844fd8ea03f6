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
struct FillPlan {
    long long item0[SPK_NOISE_MAX_LAYERS + 1];   // first work item of layer l; [n_layers] = the total
    long long off[SPK_NOISE_MAX_LAYERS];         // first float of layer l in dst
    long long hw[SPK_NOISE_MAX_LAYERS];
    unsigned long long seed;
    long long frame0;
    int n_layers, layer0, frame_step;
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
// arithmetic: the same bits for the same (seed, frame, layer, pixel).
template <bool VEC>
__global__ __launch_bounds__(THREADS) void noise_fill_kernel(float* __restrict__ dst, FillPlan pl) {
    const long long total = pl.item0[pl.n_layers];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        while (l + 1 < pl.n_layers && idx >= pl.item0[l + 1]) ++l;
        const long long hw = pl.hw[l], groups = (hw + 3) >> 2;
        const long long r = idx - pl.item0[l];
        long long b;
        if ((unsigned long long)(r | groups) >> 32) b = r / groups;
        else b = (unsigned)r / (unsigned)groups;          // (the decoder's sizes: no 64-bit division)
        const long long q = r - b * groups;
        const Bits4 bits = noise_bits(pl.seed, pl.frame0 + b * pl.frame_step, pl.layer0 + l, (uint32_t)q);
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
    SPK_REQUIRE(a, "noise_fill: null argument struct");
    SPK_REQUIRE(a->dst, "noise_fill: null dst");
    SPK_REQUIRE(a->B >= 1, "noise_fill: B must be >= 1 (got %d)", a->B);
    SPK_REQUIRE(a->n_layers >= 1 && a->n_layers <= SPK_NOISE_MAX_LAYERS, "noise_fill: n_layers must be in [1, %d] (got %d)",
                SPK_NOISE_MAX_LAYERS, a->n_layers);
    SPK_REQUIRE(a->frame0 >= 0, "noise_fill: negative frame0 (%lld)", (long long)a->frame0);
    SPK_REQUIRE(a->layer0 >= 0, "noise_fill: negative layer0 (%d)", a->layer0);
    SPK_REQUIRE(a->frame_step == 0 || a->frame_step == 1, "noise_fill: frame_step must be 0 (fixed) or 1 (fresh) (got %d)", a->frame_step);
    SPK_REQUIRE(a->frame0 <= INT64_MAX - a->B, "noise_fill: frame0 + B leaves the 63-bit frame range");
    SPK_REQUIRE(a->layer0 <= INT32_MAX - SPK_NOISE_MAX_LAYERS, "noise_fill: layer0 + n_layers leaves the 31-bit layer range");
    FillPlan pl = {};
    long long items = 0, floats = 0;
    bool vec = (uintptr_t)a->dst % 16 == 0;
    for (int l = 0; l < a->n_layers; ++l) {
        const long long hw = a->hw[l];
        SPK_REQUIRE(hw >= 1, "noise_fill: hw[%d] must be >= 1 (got %lld)", l, hw);
        SPK_REQUIRE(hw <= (1ll << 34), "noise_fill: hw[%d] = %lld is more than 2^34 pixels (the block index is 32 bits)", l, hw);
        SPK_REQUIRE(hw <= ((1ll << 46) - floats) / a->B, "noise_fill: more than 2^46 floats up to layer %d", l);
        pl.item0[l] = items;
        pl.off[l] = floats;
        pl.hw[l] = hw;
        vec = vec && hw % 4 == 0;
        items += (long long)a->B * ((hw + 3) >> 2);
        floats += (long long)a->B * hw;
    }
    pl.item0[a->n_layers] = items;
    pl.seed = a->seed;
    pl.frame0 = a->frame0;
    pl.n_layers = a->n_layers;
    pl.layer0 = a->layer0;
    pl.frame_step = a->frame_step;
    const dim3 grid((unsigned)std::min((items + THREADS - 1) / THREADS, (long long)GRID_CAP));
    if (vec) hipLaunchKernelGGL(noise_fill_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, a->dst, pl);
    else hipLaunchKernelGGL(noise_fill_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, a->dst, pl);
    return spk::check_launch("noise_fill_kernel");
}

}  // extern "C"
