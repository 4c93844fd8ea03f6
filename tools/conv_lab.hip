// Stand-alone timing of the conv kernel on the decoder's heavy layers (B = 8, production tile configs, zero data),
// without PyTorch in the process: the conv units of the library compiled into the tool, launched through spk_conv2d_fwd
// with an explicit config.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/conv_lab.hip speak-hack_amd/csrc/conv*.hip speak-hack_amd/csrc/dgrad3x3s2.hip \
//         -o tools/_bin/conv_lab && tools/_bin/conv_lab
// With -DSPK_LAB_STEPTIME the kernel stamps s_memtime after every k-step of chunk 10 of one workgroup and the tool
// prints the per-step cycle counts of its four waves (how profiles/r01_e_* located the staging costs).
#include "../speak-hack_amd/csrc/spk_common.hpp"      // (spk::err_buf(): the text behind spk_last_error)
#ifndef SPK_LAB
#define SPK_LAB 0
#endif

#include <cstdio>
#include <cstdlib>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int bench(const char* name, int config, bool ups, int B, int Cin, int Cout, int H, float* x, float* w, float* y, float* aux) {
    spk_conv2d_desc d = {};
    d.x = x; d.w_packed = w; d.y = y; d.bias = aux; d.noise_w = aux; d.noise = aux; d.style = aux;
    d.B = B; d.Cin = Cin; d.Cout = Cout; d.H = H; d.W = H; d.Hin = ups ? H / 2 : H; d.Win = d.Hin; d.kh = d.kw = 3; d.stride = 1;
    d.style_stride = 0; d.flags = SPK_EPI_BIAS | SPK_EPI_NOISE | SPK_EPI_LRELU | SPK_EPI_STYLE | (ups ? SPK_CONV_UPSAMPLE2X : 0);
    d.lrelu_slope = 0.2f; d.out_scale = 1.f; d.ksplit = 1; d.act_gain = 1.f; d.config = config;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i)
        if (spk_conv2d_fwd(&d, 0) != 0) { printf("%s: %s\n", name, spk::err_buf()); return 1; }
    CK(hipDeviceSynchronize());
    const int reps = 10;
    CK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) spk_conv2d_fwd(&d, 0);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    ms /= reps;
#ifdef SPK_LAB_STEPTIME
    {   // time stamps after every k-step of chunk 10 (workgroup 8, its four waves)
        unsigned long long* dbg; CK(hipMalloc(&dbg, 4096)); CK(hipMemset(dbg, 0, 4096));
        d.stats = reinterpret_cast<double*>(dbg);
        spk_conv2d_fwd(&d, 0);
        CK(hipDeviceSynchronize());
        unsigned long long h[256]; CK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
        for (int w = 0; w < 4; ++w) {
            printf("   wave%d step durations:", w);
            for (int k = 1; k < 64 && h[w * 64 + k]; ++k) printf(" %lld", (long long)(h[w * 64 + k] - h[w * 64 + k - 1]));
            printf("\n");
        }
        d.stats = nullptr;
        CK(hipFree(dbg));
    }
#endif
    const double fl = 2.0 * 9 * Cin * Cout * (double)H * H * B;
    spk_conv2d_form f;
    if (spk_conv2d_launch_form(&d, &f) != 0) { printf("%s: %s\n", name, spk::err_buf()); return 1; }
    printf("LAB=%d %-34s %8.1f us  %7.2f TFLOP/s   (WGs %d, LDS %lld B, tile %dx%dx%d)\n", SPK_LAB, name, ms * 1e3, fl / ms / 1e9,
           f.grid_x * f.grid_y, (long long)f.lds_bytes, f.TW, f.TH, f.TB);
    return 0;
}

int main() {
    const size_t n = (size_t)8 * 128 * 256 * 256;   // largest activation in the decoder
    float *x, *w, *y, *aux;
    CK(hipMalloc(&x, n * 4)); CK(hipMalloc(&y, n * 4)); CK(hipMalloc(&w, (size_t)64 << 20)); CK(hipMalloc(&aux, (size_t)16 << 20));
    CK(hipMemset(x, 0, n * 4)); CK(hipMemset(w, 0, (size_t)64 << 20)); CK(hipMemset(aux, 0, (size_t)16 << 20));
    int rc = 0;
    rc |= bench("64^2 256->256 plain cfg4", 4, false, 8, 256, 256, 64, x, w, y, aux);
    rc |= bench("64^2 512->256 ups cfg4", 4, true, 8, 512, 256, 64, x, w, y, aux);
    rc |= bench("128^2 128->128 plain cfg4", 4, false, 8, 128, 128, 128, x, w, y, aux);
    rc |= bench("256^2 64->64 plain cfg5", 5, false, 8, 64, 64, 256, x, w, y, aux);
    rc |= bench("256^2 128->64 ups cfg5", 5, true, 8, 128, 64, 256, x, w, y, aux);
    rc |= bench("32^2 512->512 plain cfg4 ks1", 4, false, 8, 512, 512, 32, x, w, y, aux);
    return rc;
}
