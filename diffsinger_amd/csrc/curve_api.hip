// libdsdenoise, host side of the segment front end: dsd_seconds_to_frames, dsd_curve_resample (kernels:
// curve_kernels.hip).  Handle-free like dsd_length_regulate and dsd_frame_curve, whose inputs these two produce: no
// weights, no device memory of their own.
//
// Host code only, as track_api.hip: no kernel, no HIP call, no HIP header.  The frame arithmetic and every argument check
// come before the device is selected; the device selection is api.hip's and the launches are curve_kernels.hip's, reached
// through plain functions.  So the same file compiles with a plain host compiler (tools/harness/front_harness.cpp builds
// it that way, under the sanitizers, with stand-ins for those functions).
//
// dsd_seconds_to_frames restates torch's CPU result of round(cumsum(ph_dur) / timestep + 0.5) one fp32 operation at a
// time, so nothing here may be contracted into an fma: contraction is off for the whole file.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dsdenoise.h"
#include "curve_params.h"

#ifdef __clang__
#pragma clang fp contract(off)      // a plain host compiler takes -ffp-contract=off on its command line instead
#endif

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
int select_device(const char* who, int device, bool say_range);
}  // namespace dsd
using dsd::fail;

static_assert(dsd::kCurveMax == DSD_CURVE_MAX && dsd::kCurveChunk == DSD_CURVE_CHUNK, "curve_params.h restates the header");

extern "C" {

int dsd_seconds_to_frames(const float* seconds, int32_t n, double timestep, int64_t* frames_out, int64_t* total_out) {
    const char* who = "dsd_seconds_to_frames";
    if (!seconds || !frames_out || !total_out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (n < 1) return fail(nullptr, DSD_EINVAL, "%s: n must be positive (%d)", who, n);
    const float step = (float)timestep;             // torch divides the fp32 tensor by the scalar in fp32
    if (!isfinite(timestep) || !(timestep > 0.0) || !isfinite(step) || !(step > 0.f))
        return fail(nullptr, DSD_EINVAL, "%s: timestep %.17g is not a positive finite fp32 number", who, timestep);
    double acc = 0.0;                               // torch's CPU cumsum of fp32: the running sum is a double ...
    int64_t prev = 0;
    for (int32_t i = 0; i < n; ++i) {
        const float s = seconds[i];
        if (!isfinite(s) || s < 0.f)
            return fail(nullptr, DSD_EINVAL, "%s: seconds[%d] = %g is not a finite non-negative duration", who, i, (double)s);
        acc += (double)s;
        const float c = (float)acc;                 // ... and every prefix is rounded to fp32
        const float q = c / step;                   // an fp32 divide, not a multiply by the reciprocal
        const float b = rintf(q + 0.5f);            // torch.round: half to even (the default rounding mode)
        if (!(b < 2147483648.0f))                   // also inf and NaN
            return fail(nullptr, DSD_EINVAL, "%s: boundary %d (%g frames) does not fit int32 frames", who, i, (double)b);
        const int64_t bi = (int64_t)b;
        frames_out[i] = bi - prev;
        prev = bi;
    }
    *total_out = prev;
    return DSD_OK;
}

int dsd_curve_resample(int32_t device, const dsd_curve* curves, int32_t n_curves, void* stream) {
    const char* who = "dsd_curve_resample";
    if (!curves) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (n_curves < 1 || n_curves > DSD_CURVE_MAX)
        return fail(nullptr, DSD_EINVAL, "%s: n_curves = %d outside [1, %d]", who, n_curves, DSD_CURVE_MAX);
    dsd::CurveBatch b;
    memset(&b, 0, sizeof(b));
    for (int32_t i = 0; i < n_curves; ++i) {
        const dsd_curve& c = curves[i];
        if (!c.points) return fail(nullptr, DSD_EINVAL, "%s: curve %d: points is NULL", who, i);
        if (!c.out) return fail(nullptr, DSD_EINVAL, "%s: curve %d: out is NULL", who, i);
        if (c.n_points < 2) return fail(nullptr, DSD_EINVAL, "%s: curve %d: n_points = %d (at least 2)", who, i, c.n_points);
        if (c.length < 1) return fail(nullptr, DSD_EINVAL, "%s: curve %d: length = %d (at least 1)", who, i, c.length);
        if (c.pad_to < c.length)
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: pad_to = %d below length = %d", who, i, c.pad_to, c.length);
        if (!isfinite(c.src_step) || !(c.src_step > 0.0))
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: src_step = %.17g is not positive and finite", who, i, c.src_step);
        if (!isfinite(c.dst_step) || !(c.dst_step > 0.0))
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: dst_step = %.17g is not positive and finite", who, i, c.dst_step);
        if (c.op != DSD_CURVE_PLAIN && c.op != DSD_CURVE_CLIP && c.op != DSD_CURVE_GENDER && c.op != DSD_CURVE_PITCH)
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: unknown op %d", who, i, c.op);
        if (c.op == DSD_CURVE_CLIP && !(c.lo <= c.hi))
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: CLIP needs lo <= hi (lo = %g, hi = %g)", who, i, (double)c.lo, (double)c.hi);
        if (c.op == DSD_CURVE_GENDER && !(c.lo <= 0.f && 0.f <= c.hi && isfinite(c.lo) && isfinite(c.hi)))
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: GENDER needs finite lo <= 0 <= hi (lo = %g, hi = %g)", who, i, (double)c.lo,
                        (double)c.hi);
        if (c.uv_out && c.op != DSD_CURVE_PITCH)
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: uv_out is for DSD_CURVE_PITCH only (op %d)", who, i, c.op);
        // len(np.arange(0, (n - 1) * src_step, dst_step)): the product and the quotient in double, then ceil
        const double count = ceil(((double)(c.n_points - 1) * c.src_step) / c.dst_step);
        if (!(count >= 1.0))
            return fail(nullptr, DSD_EINVAL, "%s: curve %d: src_step = %.17g over dst_step = %.17g leaves no frame", who, i, c.src_step,
                        c.dst_step);
        dsd::CurveD& d = b.c[i];
        d.points = c.points; d.out = c.out; d.uv = c.uv_out;
        d.src_step = c.src_step; d.dst_step = c.dst_step;
        d.n_points = c.n_points;
        d.valid = count < (double)c.length ? (int32_t)count : c.length;
        d.length = c.length; d.pad_to = c.pad_to; d.op = c.op;
        d.lo = c.lo; d.hi = c.hi;
        if (c.pad_to > b.max_pad) b.max_pad = c.pad_to;
        if (c.op == DSD_CURVE_PITCH) b.pitch[b.n_pitch++] = (uint8_t)i;
    }
    b.n = n_curves;
    b.log2_440 = log2(440.0);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    const char* err = dsd::launch_curve_resample(b, stream);
    return err ? fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, err) : DSD_OK;
}

}  // extern "C"
