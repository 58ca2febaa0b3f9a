// libdsdenoise, host side of a project's track: dsd_track_plan, dsd_track_place, dsd_track_peak, dsd_track_export
// (kernels: track_kernels.hip).  Handle-free like dsd_noise_fill: no weights, no device memory of its own.
//
// Host code only - no kernel, no HIP call, no HIP header: the plan and every argument check come before the device is
// selected, the device selection is api.hip's and the launches are track_kernels.hip's, reached through plain functions.
// So the same file also compiles with a plain host C++ compiler (tools/harness/track_harness.cpp builds it that way, under
// the sanitizers, with stand-ins for those functions).
#include <math.h>
#include <stdint.h>

#include "../../include/dsdenoise.h"

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
int select_device(const char* who, int device, bool say_range);
// track_kernels.hip (declared in dsd_internal.h): nullptr, or the text of the HIP error
const char* launch_track_place(double* track, long long start, long long prev_end, const float* src, long long n, void* stream);
const char* launch_track_peak(const double* track, long long total, double* peak_out, void* stream);
const char* launch_track_export(const double* track, long long total, int kind, const double* peak, void* out, void* stream);
}  // namespace dsd
using dsd::fail;

namespace {

constexpr int64_t kMaxTrack = INT32_MAX;            // samples: 13.5 hours at 44.1 kHz

bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// what dsd_track_peak and dsd_track_export ask of (track, total)
int check_track(const char* who, const double* track, int64_t total) {
    if (total < 1 || total > kMaxTrack)
        return fail(nullptr, DSD_EINVAL, "%s: total %lld outside [1, 2^31 - 1]", who, (long long)total);
    if (misaligned(track, 8)) return fail(nullptr, DSD_EINVAL, "%s: track is not 8-byte aligned", who);
    return DSD_OK;
}

int launched(const char* who, const char* err) {
    return err ? fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, err) : DSD_OK;
}

}  // namespace

extern "C" {

int dsd_track_plan(int32_t n_seg, const double* offsets_seconds, const int64_t* lengths, int32_t sample_rate,
                   int64_t* starts_out, int64_t* prev_ends_out, int64_t* total_out) {
    const char* who = "dsd_track_plan";
    if (!offsets_seconds || !lengths || !starts_out || !prev_ends_out || !total_out)
        return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (n_seg < 1) return fail(nullptr, DSD_EINVAL, "%s: n_seg must be positive (%d)", who, n_seg);
    if (sample_rate < 1) return fail(nullptr, DSD_EINVAL, "%s: sample_rate must be positive (%d)", who, sample_rate);
    int64_t end = 0;
    for (int32_t k = 0; k < n_seg; ++k) {
        const int64_t n = lengths[k];
        if (n < 1) return fail(nullptr, DSD_EINVAL, "%s: segment %d has length %lld (must be positive)", who, k, (long long)n);
        // Python's round(offset * sr): the product in double, then half to even (the default rounding mode)
        const double pos = nearbyint(offsets_seconds[k] * (double)sample_rate);
        if (!(pos >= 0.0))          // negative, or NaN
            return fail(nullptr, DSD_EINVAL, "%s: segment %d starts at sample %.0f, before the track (offset %.17g s)", who, k, pos,
                        offsets_seconds[k]);
        if (pos > (double)kMaxTrack || n > kMaxTrack || (int64_t)pos + n > kMaxTrack)
            return fail(nullptr, DSD_EINVAL, "%s: segment %d ends past 2^31 - 1 samples (start %.0f, length %lld)", who, k, pos,
                        (long long)n);
        const int64_t s = (int64_t)pos;
        if (end - s > n)
            return fail(nullptr, DSD_EINVAL, "%s: segment %d overlaps the track by %lld samples but is only %lld long", who, k,
                        (long long)(end - s), (long long)n);
        starts_out[k] = s;
        prev_ends_out[k] = end;
        end = s + n;
    }
    *total_out = end;
    return DSD_OK;
}

int dsd_track_place(int32_t device, double* track, int64_t total, int64_t start, int64_t prev_end, const float* src,
                    int64_t n, void* stream) {
    const char* who = "dsd_track_place";
    if (!track || !src) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (total < 1 || total > kMaxTrack)
        return fail(nullptr, DSD_EINVAL, "%s: total %lld outside [1, 2^31 - 1]", who, (long long)total);
    if (n < 1) return fail(nullptr, DSD_EINVAL, "%s: n must be positive (%lld)", who, (long long)n);
    if (start < 0) return fail(nullptr, DSD_EINVAL, "%s: start %lld is before the track", who, (long long)start);
    if (start > total || n > total - start)             // in this order: start + n cannot overflow
        return fail(nullptr, DSD_EINVAL, "%s: [%lld, %lld + %lld) ends past the track's %lld samples", who, (long long)start,
                    (long long)start, (long long)n, (long long)total);
    if (prev_end < 0 || prev_end > total)
        return fail(nullptr, DSD_EINVAL, "%s: prev_end %lld outside [0, %lld]", who, (long long)prev_end, (long long)total);
    if (prev_end - start > n)
        return fail(nullptr, DSD_EINVAL, "%s: the overlap of %lld samples is longer than the segment's %lld", who,
                    (long long)(prev_end - start), (long long)n);
    if (misaligned(track, 8) || misaligned(src, 4))
        return fail(nullptr, DSD_EINVAL, "%s: track must be 8-byte and src 4-byte aligned", who);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    return launched(who, dsd::launch_track_place(track, start, prev_end, src, n, stream));
}

int dsd_track_peak(int32_t device, const double* track, int64_t total, double* peak_out, void* stream) {
    const char* who = "dsd_track_peak";
    if (!track || !peak_out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (int rc = check_track(who, track, total)) return rc;
    if (misaligned(peak_out, 8)) return fail(nullptr, DSD_EINVAL, "%s: peak_out is not 8-byte aligned", who);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    return launched(who, dsd::launch_track_peak(track, total, peak_out, stream));
}

int dsd_track_export(int32_t device, const double* track, int64_t total, int32_t kind, const double* peak, void* out,
                     void* stream) {
    const char* who = "dsd_track_export";
    if (!track || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (kind != DSD_TRACK_F64 && kind != DSD_TRACK_F32 && kind != DSD_TRACK_PCM)
        return fail(nullptr, DSD_EINVAL, "%s: unknown kind %d", who, kind);
    if (peak && kind != DSD_TRACK_PCM) return fail(nullptr, DSD_EINVAL, "%s: a peak normalises DSD_TRACK_PCM only (kind %d)", who, kind);
    if (int rc = check_track(who, track, total)) return rc;
    if (misaligned(out, kind == DSD_TRACK_F64 ? 8 : kind == DSD_TRACK_F32 ? 4 : 2) || misaligned(peak, 8))
        return fail(nullptr, DSD_EINVAL, "%s: out or peak is not aligned to its element size", who);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    return launched(who, dsd::launch_track_export(track, total, kind, peak, out, stream));
}

}  // extern "C"
