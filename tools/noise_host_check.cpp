// Host-side check of csrc/noise.hip under AddressSanitizer / UBSan: the three known answers of Philox4x32-10 through
// spk_noise_bits_host (the routine the kernel compiles; the unsigned 32 x 32 -> 64-bit products and the wrapping key additions
// are where UBSan would speak up) and every refusal of spk_noise_fill (all of them happen before a launch, so no device is
// needed).  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/noise.hip tools/noise_host_check.cpp -o tools/_bin/noise_host_check
//   tools/_bin/noise_host_check
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    // (ctr; key) -> output.  ctr = (q, frame lo, layer, frame hi), key = (seed lo, seed hi): the host routine maps its arguments
    // by two's complement, so the all-ones counter is frame = layer = -1.
    const uint32_t kat[3][10] = {
        {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (const auto& k : kat) {
        const uint64_t seed = (uint64_t)k[5] << 32 | k[4], frame_bits = (uint64_t)k[3] << 32 | k[1];
        int64_t frame;
        int32_t layer;
        std::memcpy(&frame, &frame_bits, 8);
        std::memcpy(&layer, &k[2], 4);
        uint32_t out[4] = {0, 0, 0, 0};
        CHECK(spk_noise_bits_host(seed, frame, layer, k[0], out) == SPK_OK);
        CHECK(out[0] == k[6] && out[1] == k[7] && out[2] == k[8] && out[3] == k[9]);
    }
    CHECK(spk_noise_bits_host(0, 0, 0, 0, nullptr) == SPK_EINVAL);

    // spk_noise_fill: every bad argument is refused before anything is launched (dst is a host array: never written)
    float f[8];
    auto good = [&]() {
        spk_noise_fill_args a;
        std::memset(&a, 0, sizeof a);
        a.dst = f;
        a.seed = 1;
        a.B = 1;
        a.frame_step = 1;
        a.n_layers = 2;
        a.hw[0] = 4;
        a.hw[1] = 3;
        return a;
    };
    spk_noise_fill_args a;
    CHECK(spk_noise_fill(nullptr, nullptr) == SPK_EINVAL);
    a = good(); a.dst = nullptr;                   CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "dst"));
    a = good(); a.B = 0;                           CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "B must"));
    a = good(); a.B = -3;                          CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL);
    a = good(); a.n_layers = 0;                    CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "n_layers"));
    a = good(); a.n_layers = SPK_NOISE_MAX_LAYERS + 1; CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "n_layers"));
    a = good(); a.n_layers = -1;                   CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL);
    a = good(); a.hw[1] = 0;                       CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "hw[1]"));
    a = good(); a.hw[0] = -4;                      CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "hw[0]"));
    a = good(); a.hw[0] = (1ll << 34) + 1;         CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "2^34"));
    a = good(); a.n_layers = SPK_NOISE_MAX_LAYERS; CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "hw[2]"));
    a = good(); a.frame0 = -1;                     CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "frame0"));
    a = good(); a.frame0 = INT64_MAX;              CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "frame0"));
    a = good(); a.layer0 = -1;                     CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "layer0"));
    a = good(); a.layer0 = INT32_MAX;              CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "layer0"));
    a = good(); a.frame_step = -1;                 CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "frame_step"));
    a = good(); a.frame_step = 2;                  CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "frame_step"));
    a = good(); a.B = INT32_MAX; a.hw[0] = 1ll << 34; a.hw[1] = 1ll << 34;   // the float count is checked in 64 bits, layer by layer
    CHECK(spk_noise_fill(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "2^46"));
    std::printf("noise host check: 3 known answers and the argument refusals passed\n");
    return 0;
}
