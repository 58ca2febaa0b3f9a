// What curve_api.hip (host code only, no HIP header) hands to curve_kernels.hip: the checked descriptors of one
// dsd_curve_resample call, as they travel in the launch arguments.  Plain C++, so the host file also compiles with a plain
// host compiler (tools/harness/front_harness.cpp).
#pragma once
#include <stdint.h>

namespace dsd {

constexpr int kCurveMax = 32;       // DSD_CURVE_MAX
constexpr int kCurveChunk = 256;    // DSD_CURVE_CHUNK: frames per workgroup and step of the PITCH walk

struct CurveD {
    const float* points;
    float* out;
    uint8_t* uv;
    double src_step, dst_step;
    int32_t n_points;
    int32_t valid;                  // min(count, length) >= 1: frames computed from the points; the rest hold frame valid - 1
    int32_t length, pad_to, op;
    float lo, hi;
};

struct CurveBatch {
    CurveD c[kCurveMax];
    double log2_440;                // the host's log2(440.0), as numpy's hz_to_midi takes it
    int32_t n, max_pad;             // curves; the largest pad_to
    int32_t n_pitch;
    uint8_t pitch[kCurveMax];       // indices of the DSD_CURVE_PITCH curves
};
static_assert(sizeof(CurveBatch) <= 3072, "the descriptors travel in the kernel arguments (4 KiB at most)");

// curve_kernels.hip: nullptr, or the text of the HIP error.  One launch; a second one when n_pitch > 0.
const char* launch_curve_resample(const CurveBatch& b, void* stream);

}  // namespace dsd
