// libdsdenoise, host side of the duration-to-frame stages: dsd_length_regulate, dsd_frame_curve (kernels:
// frames_kernels.hip).  Both are handle-free like dsd_cond_assemble: no weights, no device memory of their own.
#include "api_host.h"

int dsd_length_regulate(int32_t device, const int64_t* dur, int32_t B, int32_t L, int32_t T, int64_t* mel2x, void* stream) {
    const char* who = "dsd_length_regulate";
    if (!dur || !mel2x) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (B < 1 || L < 1) return fail(nullptr, DSD_EINVAL, "%s: B and L must be positive (B=%d, L=%d)", who, B, L);
    if (L > kRegulateMaxTokens)
        return fail(nullptr, DSD_EINVAL, "%s: L = %d exceeds the %d tokens an encoder takes", who, L, kRegulateMaxTokens);
    if (T < 1) return fail(nullptr, DSD_EINVAL, "%s: T must be positive (got %d)", who, T);
    if (int rc = select_device(who, device, false)) return rc;
    hipError_t e = launch_length_regulate((const long long*)dur, B, L, T, (long long*)mel2x, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return DSD_OK;
}

int dsd_frame_curve(int32_t device, const float* note_midi, const int64_t* mel2note, const float* pitch,
                    const uint8_t* retake, int32_t B, int32_t N, int32_t T, const int32_t* lengths, const float* weights,
                    int32_t K, float* base_out, float* blend_out, float* delta_out, void* stream) {
    const char* who = "dsd_frame_curve";
    if (!note_midi || !mel2note || !pitch || !retake || !weights || !base_out || !blend_out || !delta_out)
        return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (B < 1 || N < 1 || T < 1) return fail(nullptr, DSD_EINVAL, "%s: B, N and T must be positive (%d, %d, %d)", who, B, N, T);
    if (K < 1 || K > kCurveMaxTaps) return fail(nullptr, DSD_EINVAL, "%s: K = %d outside [1, %d]", who, K, kCurveMaxTaps);
    if (lengths)
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 0 || lengths[b] > T)
                return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d outside [0, T = %d]", who, b, lengths[b], T);
    if (int rc = select_device(who, device, false)) return rc;
    FrameCurveP p;
    memset(&p, 0, sizeof(p));
    p.note_midi = note_midi; p.mel2note = (const long long*)mel2note; p.pitch = pitch; p.retake = retake;
    p.base = base_out; p.blend = blend_out; p.delta = delta_out;
    p.N = N; p.T = T; p.K = K;
    memcpy(p.w, weights, sizeof(float) * K);
    for (int b0 = 0; b0 < B; b0 += kCurveItems) {
        const int items = std::min(kCurveItems, B - b0);
        p.b0 = b0;
        for (int b = 0; b < items; ++b) p.len[b] = lengths ? lengths[b0 + b] : T;
        hipError_t e = launch_frame_curve(p, items, (hipStream_t)stream);
        if (e != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    }
    return DSD_OK;
}
