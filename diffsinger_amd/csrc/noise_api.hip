// libdsdenoise, host side of the seeded draws: dsd_noise_fill (kernel: noise_kernels.hip).  Handle-free like
// dsd_length_regulate: no weights, no device memory of its own, nothing but launches on the caller's stream.
#include "api_host.h"

int dsd_noise_fill(int32_t device, const dsd_noise_spec* spec, float* out, void* stream) {
    const char* who = "dsd_noise_fill";
    if (!spec || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (spec->struct_size != (int32_t)sizeof(dsd_noise_spec))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, spec->struct_size, sizeof(dsd_noise_spec));
    if (!spec->seeds) return fail(nullptr, DSD_EINVAL, "%s: null seeds", who);
    if (spec->kind != DSD_NOISE_NORMAL && spec->kind != DSD_NOISE_UNIFORM)
        return fail(nullptr, DSD_EINVAL, "%s: unknown kind %d", who, spec->kind);
    if (spec->n < 1 || spec->B < 1 || spec->rows < 1 || spec->cols < 1)
        return fail(nullptr, DSD_EINVAL, "%s: n, B, rows and cols must be positive (%d, %d, %d, %d)", who, spec->n, spec->B,
                    spec->rows, spec->cols);
    int64_t elems = 1;                      // factor by factor: each partial product stays below 2^62
    for (int64_t f : {(int64_t)spec->n, (int64_t)spec->B, (int64_t)spec->rows, (int64_t)spec->cols}) {
        elems *= f;
        if (elems > INT32_MAX)
            return fail(nullptr, DSD_EINVAL, "%s: [%d, %d, %d, %d] holds more than 2^31 - 1 elements", who, spec->n, spec->B,
                        spec->rows, spec->cols);
    }
    if (int rc = select_device(who, device, false)) return rc;
    NoiseP p;
    memset(&p, 0, sizeof(p));
    p.out = out; p.src = spec->src; p.scale = spec->scale; p.src_scale = spec->src_scale;
    p.domain = spec->domain; p.first_stream = (unsigned)spec->first_stream;
    p.n = spec->n; p.B = spec->B; p.rows = spec->rows; p.cols = spec->cols; p.kind = spec->kind;
    for (int b0 = 0; b0 < spec->B; b0 += kNoiseItems) {
        const int items = std::min(kNoiseItems, spec->B - b0);
        p.b0 = b0;
        for (int b = 0; b < items; ++b) p.seed[b] = spec->seeds[b0 + b];
        hipError_t e = launch_noise_fill(p, items, (hipStream_t)stream);
        if (e != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    }
    return DSD_OK;
}
