// libdsdenoise, host side of validation scoring: dsd_diffuse, dsd_masked_loss, dsd_curve_stats, dsd_dur_score (kernels:
// score_kernels.hip).  Handle-free like dsd_noise_fill: no weights, no device memory of its own (the partial sums live in
// the caller's workspace), nothing but launches on the caller's stream.  Every argument check comes before the device is
// selected.
#include "api_host.h"

static_assert(kScoreSlots * kScoreMaxBlocks * 8 == DSD_SCORE_WORKSPACE_BYTES, "the header's workspace constant");

namespace {

bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// the product of the factors, or -1 past 2^31 - 1 (factor by factor: each partial product stays below 2^62)
int64_t elements(std::initializer_list<int64_t> factors) {
    int64_t n = 1;
    for (int64_t f : factors) {
        n *= f;
        if (n > INT32_MAX) return -1;
    }
    return n;
}

int launched(const char* who, hipError_t e) {
    return e == hipSuccess ? DSD_OK : fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace

int dsd_diffuse(int32_t device, const dsd_diffuse_spec* spec, float* x_t, float* target, void* stream) {
    const char* who = "dsd_diffuse";
    if (!spec || !x_t) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (spec->struct_size != (int32_t)sizeof(dsd_diffuse_spec))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, spec->struct_size, sizeof(dsd_diffuse_spec));
    if (spec->kind != DSD_DIFFUSE_DDPM && spec->kind != DSD_DIFFUSE_REFLOW)
        return fail(nullptr, DSD_EINVAL, "%s: unknown kind %d", who, spec->kind);
    if (!spec->x0 || !spec->a) return fail(nullptr, DSD_EINVAL, "%s: null x0 or a", who);
    if (spec->kind == DSD_DIFFUSE_DDPM && !spec->c) return fail(nullptr, DSD_EINVAL, "%s: DSD_DIFFUSE_DDPM needs c", who);
    if (!spec->eps && !spec->seeds) return fail(nullptr, DSD_EINVAL, "%s: neither eps nor seeds", who);
    if (!target && (!spec->eps || spec->kind != DSD_DIFFUSE_DDPM))
        return fail(nullptr, DSD_EINVAL, "%s: target may be NULL only with a given eps and DSD_DIFFUSE_DDPM", who);
    if (spec->B < 1 || spec->rows < 1 || spec->cols < 1)
        return fail(nullptr, DSD_EINVAL, "%s: B, rows and cols must be positive (%d, %d, %d)", who, spec->B, spec->rows, spec->cols);
    if (elements({spec->B, spec->rows, spec->cols}) < 0)
        return fail(nullptr, DSD_EINVAL, "%s: [%d, %d, %d] holds more than 2^31 - 1 elements", who, spec->B, spec->rows, spec->cols);
    if (x_t == target || x_t == spec->x0 || x_t == spec->eps || (target && (target == spec->x0 || target == spec->eps)))
        return fail(nullptr, DSD_EINVAL, "%s: an output must not be an input or the other output", who);
    if (misaligned(x_t, 4) || misaligned(target, 4) || misaligned(spec->x0, 4) || misaligned(spec->eps, 4) || misaligned(spec->a, 4) ||
        misaligned(spec->c, 4))
        return fail(nullptr, DSD_EINVAL, "%s: a pointer is not 4-byte aligned", who);
    if (int rc = select_device(who, device, false)) return rc;
    DiffuseP p;
    memset(&p, 0, sizeof(p));
    p.x_t = x_t; p.target = target; p.x0 = spec->x0; p.eps = spec->eps; p.a = spec->a; p.c = spec->c;
    p.domain = spec->domain; p.rows = spec->rows; p.cols = spec->cols; p.kind = spec->kind;
    for (int b0 = 0; b0 < spec->B; b0 += kNoiseItems) {
        const int items = std::min(kNoiseItems, spec->B - b0);
        p.b0 = b0;
        if (!spec->eps)
            for (int b = 0; b < items; ++b) p.seed[b] = spec->seeds[b0 + b];
        if (int rc = launched(who, launch_diffuse(p, items, (hipStream_t)stream))) return rc;
    }
    return DSD_OK;
}

int dsd_masked_loss(int32_t device, const dsd_loss_spec* spec, void* workspace, double* out, void* stream) {
    const char* who = "dsd_masked_loss";
    if (!spec || !workspace || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (spec->struct_size != (int32_t)sizeof(dsd_loss_spec))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, spec->struct_size, sizeof(dsd_loss_spec));
    if (spec->kind != DSD_LOSS_L1 && spec->kind != DSD_LOSS_L2) return fail(nullptr, DSD_EINVAL, "%s: unknown kind %d", who, spec->kind);
    if (!spec->pred || !spec->target) return fail(nullptr, DSD_EINVAL, "%s: null pred or target", who);
    if (spec->B < 1 || spec->rows < 1 || spec->cols < 1)
        return fail(nullptr, DSD_EINVAL, "%s: B, rows and cols must be positive (%d, %d, %d)", who, spec->B, spec->rows, spec->cols);
    if (elements({spec->B, spec->rows, spec->cols}) < 0)
        return fail(nullptr, DSD_EINVAL, "%s: [%d, %d, %d] holds more than 2^31 - 1 elements", who, spec->B, spec->rows, spec->cols);
    if (misaligned(workspace, 8) || misaligned(out, 8) || misaligned(spec->pred, 4) || misaligned(spec->target, 4) ||
        misaligned(spec->non_padding, 4) || misaligned(spec->t, 4))
        return fail(nullptr, DSD_EINVAL, "%s: workspace and out must be 8-byte, the tensors 4-byte aligned", who);
    if (int rc = select_device(who, device, false)) return rc;
    LossP p;
    p.pred = spec->pred; p.target = spec->target; p.non_padding = spec->non_padding; p.t = spec->t;
    p.B = spec->B; p.rows = spec->rows; p.cols = spec->cols; p.kind = spec->kind;
    return launched(who, launch_masked_loss(p, workspace, out, (hipStream_t)stream));
}

int dsd_curve_stats(int32_t device, const float* pred, const float* target, const uint8_t* mask, int64_t n, float tolerance,
                    void* workspace, dsd_curve_result* out, void* stream) {
    const char* who = "dsd_curve_stats";
    if (!pred || !target || !workspace || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (n < 1 || n > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: n %lld outside [1, 2^31 - 1]", who, (long long)n);
    if (misaligned(workspace, 8) || misaligned(out, 8) || misaligned(pred, 4) || misaligned(target, 4))
        return fail(nullptr, DSD_EINVAL, "%s: workspace and out must be 8-byte, the curves 4-byte aligned", who);
    if (int rc = select_device(who, device, false)) return rc;
    return launched(who, launch_curve_stats(pred, target, mask, n, tolerance, workspace, out, (hipStream_t)stream));
}

int dsd_dur_score(int32_t device, const dsd_dur_spec* spec, float* wdur_pred, float* wdur_gt, void* workspace,
                  dsd_dur_result* out, void* stream) {
    const char* who = "dsd_dur_score";
    if (!spec || !wdur_pred || !wdur_gt || !workspace || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (spec->struct_size != (int32_t)sizeof(dsd_dur_spec))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, spec->struct_size, sizeof(dsd_dur_spec));
    if (spec->kind != DSD_DUR_MSE && spec->kind != DSD_DUR_HUBER) return fail(nullptr, DSD_EINVAL, "%s: unknown kind %d", who, spec->kind);
    if (!spec->dur_pred || !spec->dur_gt || !spec->ph2word) return fail(nullptr, DSD_EINVAL, "%s: null dur_pred, dur_gt or ph2word", who);
    if (spec->B < 1 || spec->L < 1) return fail(nullptr, DSD_EINVAL, "%s: B and L must be positive (%d, %d)", who, spec->B, spec->L);
    if (spec->n_words < 2)
        return fail(nullptr, DSD_EINVAL, "%s: n_words %d: ph2word.max() + 1 of at least one word expected", who, spec->n_words);
    if (elements({spec->B, (int64_t)spec->L + spec->n_words}) < 0)
        return fail(nullptr, DSD_EINVAL, "%s: B * (L + n_words) = %d * (%d + %d) is more than 2^31 - 1 elements", who, spec->B, spec->L,
                    spec->n_words);
    if (wdur_pred == wdur_gt || (const float*)wdur_pred == spec->dur_pred || (const float*)wdur_pred == spec->dur_gt ||
        (const float*)wdur_gt == spec->dur_pred || (const float*)wdur_gt == spec->dur_gt)
        return fail(nullptr, DSD_EINVAL, "%s: an output must not be an input or the other output", who);
    if (misaligned(workspace, 8) || misaligned(out, 8) || misaligned(spec->ph2word, 8) || misaligned(spec->dur_pred, 4) ||
        misaligned(spec->dur_gt, 4) || misaligned(wdur_pred, 4) || misaligned(wdur_gt, 4))
        return fail(nullptr, DSD_EINVAL, "%s: workspace, out and ph2word must be 8-byte, the float tensors 4-byte aligned", who);
    if (int rc = select_device(who, device, false)) return rc;
    DurP p;
    p.dur_pred = spec->dur_pred; p.dur_gt = spec->dur_gt; p.ph2word = (const long long*)spec->ph2word; p.mask = spec->mask;
    p.wdur_pred = wdur_pred; p.wdur_gt = wdur_gt;
    p.B = spec->B; p.L = spec->L; p.n_words = spec->n_words; p.kind = spec->kind;
    p.offset = spec->offset; p.tol_rhythm = spec->rhythm_tolerance; p.tol_pdur = spec->pdur_tolerance;
    return launched(who, launch_dur_score(p, workspace, out, (hipStream_t)stream));
}
