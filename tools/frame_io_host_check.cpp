// Host-side check of csrc/frame_io.hip under AddressSanitizer / UBSan: the resize-table builder at the sizes the tests and the
// benchmark use (tables sized exactly, so a write past a row or a table is caught) and the argument validation of the two
// entry points (every refusal happens before a launch, so no device is needed).  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_io.hip tools/frame_io_host_check.cpp -o tools/_bin/frame_io_host_check
//   tools/_bin/frame_io_host_check
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_check.hpp"

int main() {
    const int sizes[][2] = {{37, 16}, {53, 16}, {135, 32}, {240, 32}, {20, 32}, {28, 32}, {32, 32}, {2, 1}, {1, 4}, {1, 1},
                            {1080, 256}, {1920, 256}, {24, 768}, {4096, 3}, {3, 4096}};
    for (const auto& sz : sizes) {
        const int n_in = sz[0], n_out = sz[1];
        const int taps = spk_resize_table_taps(n_in, n_out);
        CHECK(taps >= 1 && taps <= n_in);
        std::vector<int32_t> first(n_out), count(n_out);
        std::vector<double> w((size_t)n_out * taps);
        std::vector<float> w32((size_t)n_out * taps);
        CHECK(spk_resize_table(n_in, n_out, taps, first.data(), count.data(), w.data(), w32.data()) == SPK_OK);
        CHECK(spk_resize_table(n_in, n_out, taps, first.data(), count.data(), nullptr, w32.data()) == SPK_OK);
        int widest = 0;
        for (int o = 0; o < n_out; ++o) {
            CHECK(count[o] >= 1 && first[o] >= 0 && first[o] + count[o] <= n_in);
            widest = count[o] > widest ? count[o] : widest;
            double s = 0.0, s32 = 0.0;
            for (int j = 0; j < taps; ++j) {
                CHECK(j < count[o] ? w[(size_t)o * taps + j] >= 0.0 : (w[(size_t)o * taps + j] == 0.0 && w32[(size_t)o * taps + j] == 0.f));
                s += w[(size_t)o * taps + j];
                s32 += (double)w32[(size_t)o * taps + j];
            }
            CHECK(std::fabs(s - 1.0) < 1e-14 && s32 == 1.0);
        }
        CHECK(widest == taps);
        if (taps > 1) CHECK(spk_resize_table(n_in, n_out, taps - 1, first.data(), count.data(), w.data(), nullptr) == SPK_EINVAL);
    }
    CHECK(spk_resize_table_taps(0, 1) == SPK_EINVAL && spk_resize_table_taps(1, 0) == SPK_EINVAL);
    int32_t i4[4];
    double d4[4];
    CHECK(spk_resize_table(4, 4, 1, nullptr, i4, d4, nullptr) == SPK_EINVAL);
    CHECK(spk_resize_table(4, 4, 1, i4, i4, nullptr, nullptr) == SPK_EINVAL);
    CHECK(spk_resize_table(4, 4, 0, i4, i4, d4, nullptr) == SPK_EINVAL);

    // the two launchers: every bad argument is refused before anything is dereferenced or launched
    uint8_t u8[4];
    float f[4];
    const uint8_t* src = u8;
    const int32_t* tab = i4;
    auto to_f32 = [&](const uint8_t* s, float* d, const int32_t* t, const float* w, int N, int Hin, int Win, int64_t row, int taps, int Hout, int Wout) {
        return spk_frames_u8_to_f32(s, row * Hin, row, N, Hin, Win, 0, t, t, w, taps, t, t, w, taps, d, Hout, Wout, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    CHECK(to_f32(nullptr, f, tab, f, 1, 4, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, nullptr, tab, f, 1, 4, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, nullptr, f, 1, 4, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, nullptr, 1, 4, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 0, 4, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 0, 4, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 4, 0, 12, 2, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 4, 4, 12, 0, 2, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 4, 4, 12, 2, 0, 2) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 4, 4, 12, 2, 2, -1) == SPK_EINVAL);
    CHECK(to_f32(src, f, tab, f, 1, 4, 4, 11, 2, 2, 2) == SPK_EINVAL && std::strstr(spk_last_error(), "row stride"));
    CHECK(to_f32(src, f, tab, f, 1, 4, 0x7fffffff, 12, 2, 2, 2) == SPK_EINVAL);       // 3 * Win does not wrap
    CHECK(spk_frames_f32_to_u8(nullptr, u8, 1, 1, 1, 0, -1.f, 127.5f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, nullptr, 1, 1, 1, 0, -1.f, 127.5f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, u8, 0, 1, 1, 0, -1.f, 127.5f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, u8, 1, 0, 1, 0, -1.f, 127.5f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, u8, 1, 1, 0, 0, -1.f, 127.5f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, u8, 1, 1, 1, 0, -1.f, 0.f, nullptr) == SPK_EINVAL);
    CHECK(spk_frames_f32_to_u8(f, u8, 1, 1, 1, 0, NAN, 127.5f, nullptr) == SPK_EINVAL);
    std::printf("frame_io host check: %zu table sizes and the argument refusals passed\n", sizeof(sizes) / sizeof(sizes[0]));
    return 0;
}
