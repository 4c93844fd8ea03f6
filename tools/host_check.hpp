// What the stand-alone host checks (tools/*_host_check.cpp) share.  Each links one csrc/*.hip file alone, so it brings its own
// spk_last_error -- the library defines that next to its other kernels (csrc/pointwise.hip) -- and CHECK, which ends main() with
// the line, the condition and the library's last error message.
#pragma once

#include <cstdio>

#include "../speak-hack_amd/csrc/spk_common.hpp"

extern "C" const char* spk_last_error(void) { return spk::err_buf(); }

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, spk_last_error()); \
            return 1;                                                      \
        }                                                                  \
    } while (0)
