// libdsdenoise, the host-only half of the acoustic twin: what a DSD_ACOUSTIC_TABLES section must hold for its config, what
// the inner sections' configs must say (both behind dsd_acoustic_open, acoustic_api.hip), and dsd_acoustic_plan.  No kernel,
// no HIP call, no HIP header - like variance_tables.hip, so tools/harness/acoustic_harness.cpp compiles this file with a
// plain host compiler under the sanitizers.  Everything here runs before dsd_acoustic_open touches a device.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <exception>
#include <vector>

#include "acoustic_tables.h"

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);

namespace {

const char* const WHO = "dsd_acoustic_open";

struct Want {
    const char* name;
    int64_t shape[2];
    int ndim;
    bool allowed;       // false: the config excludes it
    bool optional;      // with allowed: may be absent
    int* slot;
};

int find(const dsd_model_tensor_info* t, int32_t n, const char* name) {
    for (int32_t j = 0; j < n; ++j)
        if (t[j].name && strcmp(t[j].name, name) == 0) return j;
    return -1;
}

bool is_flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace

int acoustic_tables_check(const dsd_acoustic_config* c, int32_t cfg_size, const dsd_model_tensor_info* tensors, int32_t n_tensors,
                          const char* section, AcousticTableIndex* index) {
    if (!c || !section || !index || (n_tensors > 0 && !tensors)) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
    if (cfg_size != (int32_t)sizeof(dsd_acoustic_config) || c->struct_size != (int32_t)sizeof(dsd_acoustic_config))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": struct_size %d (config of %d bytes) != %zu", WHO, section,
                    cfg_size == (int32_t)sizeof(dsd_acoustic_config) ? c->struct_size : -1, cfg_size, sizeof(dsd_acoustic_config));
    const struct { const char* name; int32_t v; } flags[] = {
        {"use_lang_id", c->use_lang_id}, {"use_spk_id", c->use_spk_id}, {"f0_discrete", c->f0_discrete},
        {"use_shallow_diffusion", c->use_shallow_diffusion}, {"mel_base_e", c->mel_base_e}};
    for (const auto& f : flags)
        if (!is_flag(f.v)) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": %s = %d is neither 0 nor 1", WHO, section, f.name, f.v);
    if (c->hidden_size < 1 || c->vocab_size < 1 || c->out_dims < 1)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": hidden_size %d, vocab_size %d and out_dims %d must be positive", WHO, section,
                    c->hidden_size, c->vocab_size, c->out_dims);
    if (c->embed_flags >= (DSD_EMBED_SPEED << 1))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": embed_flags = 0x%x has a bit above DSD_EMBED_SPEED", WHO, section, c->embed_flags);
    if (c->use_lang_id ? c->num_lang < 1 : c->num_lang != 0)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_lang_id = %d with num_lang = %d", WHO, section, c->use_lang_id, c->num_lang);
    if (c->use_spk_id ? c->num_spk < 1 : c->num_spk != 0)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_spk_id = %d with num_spk = %d", WHO, section, c->use_spk_id, c->num_spk);
    if ((c->embed_flags & DSD_EMBED_KEY_SHIFT) && !(c->shift_min <= 0.f && 0.f <= c->shift_max))       // a NaN fails too
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": shift_min = %g <= 0 <= shift_max = %g does not hold", WHO, section,
                    (double)c->shift_min, (double)c->shift_max);
    if ((c->embed_flags & DSD_EMBED_SPEED) && !(0.f < c->speed_min && c->speed_min <= c->speed_max))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": 0 < speed_min = %g <= speed_max = %g does not hold", WHO, section,
                    (double)c->speed_min, (double)c->speed_max);
    if (c->diffusion_type == DSD_DIFFUSE_DDPM) {
        if (c->timesteps < 1 || c->k_step < 0 || c->k_step > c->timesteps)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": timesteps = %d, k_step = %d (0 <= k_step <= timesteps, timesteps >= 1)", WHO,
                        section, c->timesteps, c->k_step);
        if (c->schedule_type != DSD_SCHEDULE_LINEAR && c->schedule_type != DSD_SCHEDULE_COSINE)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": schedule_type = %d", WHO, section, c->schedule_type);
        if (c->schedule_type == DSD_SCHEDULE_LINEAR && !(c->max_beta > 0.0 && c->max_beta < 1.0))
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": max_beta = %g outside (0, 1)", WHO, section, c->max_beta);
    } else if (c->diffusion_type == DSD_DIFFUSE_REFLOW) {
        if (!(c->t_start >= 0.f && c->t_start <= 1.f))
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": t_start = %g outside [0, 1]", WHO, section, (double)c->t_start);
        if (!(c->time_scale_factor > 0.f))
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": time_scale_factor = %g must be positive", WHO, section, (double)c->time_scale_factor);
    } else {
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": diffusion_type = %d", WHO, section, c->diffusion_type);
    }

    AcousticTableIndex& ix = *index;
    memset(&ix, 0xFF, sizeof(ix));          // every slot -1
    ix.mask_any = 0;
    const Want want[] = {
        {"cross_lingual_mask", {c->vocab_size, -1}, 1, true, false, &ix.mask},
        {"spec_min", {c->out_dims, -1}, 1, true, false, &ix.spec_min},
        {"spec_max", {c->out_dims, -1}, 1, true, false, &ix.spec_max},
        {"fs2.pitch_embed.weight", {DSD_AC_PITCH_BINS, c->hidden_size}, 2, c->f0_discrete != 0, false, &ix.pitch_embed},
        {"frozen_spk_embed", {c->hidden_size, -1}, 1, c->use_spk_id != 0, true, &ix.frozen_spk},
        {"frozen_key_shift", {1, -1}, 1, (c->embed_flags & DSD_EMBED_KEY_SHIFT) != 0, true, &ix.frozen_key_shift},
    };
    const int nw = (int)(sizeof(want) / sizeof(want[0]));
    int matched = 0;
    for (int k = 0; k < nw; ++k) {
        const Want& w = want[k];
        const int j = find(tensors, n_tensors, w.name);
        if (j < 0) {
            if (w.allowed && !w.optional) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" lacks the tensor \"%s\" its config requires", WHO, section, w.name);
            continue;
        }
        if (!w.allowed) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" carries the tensor \"%s\", which its config excludes", WHO, section, w.name);
        const dsd_model_tensor_info& t = tensors[j];
        bool same = t.ndim == w.ndim && t.data != nullptr;
        for (int d = 0; same && d < w.ndim; ++d) same = t.shape[d] == w.shape[d];
        if (!same) {
            if (w.ndim == 2)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": tensor \"%s\" must be [%lld, %lld] (stored: %d dims, [%lld, %lld])", WHO, section,
                            w.name, (long long)w.shape[0], (long long)w.shape[1], t.ndim, (long long)t.shape[0], (long long)t.shape[1]);
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": tensor \"%s\" must be [%lld] (stored: %d dims, [%lld])", WHO, section, w.name,
                        (long long)w.shape[0], t.ndim, (long long)t.shape[0]);
        }
        *w.slot = j;
        ++matched;
    }
    if (matched != n_tensors)           // names are unique in a section (dsd_model_open), so one is left over
        for (int32_t j = 0; j < n_tensors; ++j) {
            bool known = false;
            for (int k = 0; k < nw && !known; ++k) known = tensors[j].name && strcmp(tensors[j].name, want[k].name) == 0;
            if (!known)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" carries the tensor \"%s\", which the acoustic model's tables do not have", WHO,
                            section, tensors[j].name ? tensors[j].name : "(null)");
        }
    const float* mask = tensors[ix.mask].data;
    for (int64_t i = 0; i < c->vocab_size; ++i) {
        if (mask[i] != 0.f && mask[i] != 1.f)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": cross_lingual_mask[%lld] = %g is neither 0 nor 1", WHO, section, (long long)i, (double)mask[i]);
        if (mask[i] == 1.f) ix.mask_any = 1;
    }
    const float *lo = tensors[ix.spec_min].data, *hi = tensors[ix.spec_max].data;
    for (int64_t m = 0; m < c->out_dims; ++m)
        if (!(hi[m] > lo[m]) || !isfinite(hi[m]) || !isfinite(lo[m]))
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": spec_max[%lld] = %g is not above spec_min[%lld] = %g (both finite)", WHO, section,
                        (long long)m, (double)hi[m], (long long)m, (double)lo[m]);
    return DSD_OK;
}

int acoustic_inner_check(const dsd_acoustic_config* c, const dsd_encoder_config* fs2, const dsd_config* denoiser, const dsd_config* aux) {
    if (!c || !fs2 || !denoiser || (c->use_shallow_diffusion && !aux)) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
#define SAME(have, want, lhs, rhs)                                                                                           \
    if ((have) != (want)) return fail(nullptr, DSD_EINVAL, "%s: " lhs " = %d does not match " rhs " = %d", WHO, (int)(have), (int)(want))
    SAME(fs2->hidden_size, c->hidden_size, "fs2.hidden_size", "tables.hidden_size");
    SAME(fs2->vocab_size, c->vocab_size, "fs2.vocab_size", "tables.vocab_size");
    SAME(fs2->embed_flags, c->embed_flags, "fs2.embed_flags", "tables.embed_flags");
    SAME(fs2->num_spk, c->num_spk, "fs2.num_spk", "tables.num_spk");
    SAME(fs2->num_lang, c->num_lang, "fs2.num_lang", "tables.num_lang");
    SAME(denoiser->in_dims, c->out_dims, "denoiser.in_dims", "tables.out_dims");
    SAME(denoiser->n_feats, 1, "denoiser.n_feats", "the one spectrogram of an acoustic model, n_feats");
    SAME(denoiser->hidden_size, c->hidden_size, "denoiser.hidden_size", "tables.hidden_size");
    if (c->use_shallow_diffusion) {
        SAME(aux->in_dims, c->out_dims, "aux.in_dims", "tables.out_dims");
        SAME(aux->n_feats, 1, "aux.n_feats", "the one spectrogram of an acoustic model, n_feats");
        SAME(aux->hidden_size, c->hidden_size, "aux.hidden_size", "tables.hidden_size");
    }
#undef SAME
    return DSD_OK;
}

}  // namespace dsd

using namespace dsd;

extern "C" int dsd_acoustic_plan(const dsd_acoustic_config* c, float depth, int32_t steps, dsd_acoustic_plan_t* out) {
    const char* who = "dsd_acoustic_plan";
    if (!c || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    if (c->struct_size != (int32_t)sizeof(dsd_acoustic_config))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, c->struct_size, sizeof(dsd_acoustic_config));
    if (depth != depth) return fail(nullptr, DSD_EINVAL, "%s: depth is NaN", who);
    dsd_acoustic_plan_t p;
    memset(&p, 0, sizeof(p));
    p.mode = c->diffusion_type;
    p.steps = steps;
    p.start = DSD_AC_START_NOISE;
    p.src_scale = 0.f;
    p.noise_scale = 1.f;
    const bool source = depth >= 0.f;
    if (c->diffusion_type == DSD_DIFFUSE_DDPM) {
        if (steps < 1) return fail(nullptr, DSD_EINVAL, "%s: steps = %d must be positive for DDPM", who, steps);
        if (c->timesteps < 1 || c->k_step < 0 || c->k_step > c->timesteps)
            return fail(nullptr, DSD_EINVAL, "%s: timesteps = %d, k_step = %d", who, c->timesteps, c->k_step);
        try {
            std::vector<int64_t> factors;
            for (int32_t i = 1; i <= c->timesteps; ++i)
                if (c->timesteps % i == 0) factors.push_back(i);
            if (int rc = dsd_onnx_ddpm_plan(c->timesteps, c->k_step, factors.data(), (int32_t)factors.size(), steps, source ? (double)depth : -1.0,
                                            &p.t_max, &p.speedup))
                return rc;
            if (source && p.t_max < c->timesteps) {
                if (p.t_max > 0) {
                    std::vector<float> tables((size_t)DSD_DDPM_TABLES * (size_t)c->timesteps);
                    if (int rc = dsd_ddpm_tables_fill(c->schedule_type, c->timesteps, c->max_beta, tables.data())) return rc;
                    p.start = DSD_AC_START_MIX;
                    p.src_scale = tables[(size_t)3 * c->timesteps + (size_t)(p.t_max - 1)];       // sqrt_alphas_cumprod
                    p.noise_scale = tables[(size_t)4 * c->timesteps + (size_t)(p.t_max - 1)];     // sqrt_one_minus_alphas_cumprod
                } else {
                    p.start = DSD_AC_START_SOURCE;
                    p.src_scale = 1.f;
                    p.noise_scale = 0.f;
                }
            }
        } catch (const std::exception&) {
            return fail(nullptr, DSD_ENOMEM, "%s: out of host memory", who);
        }
        p.n_step_noise = p.speedup == 1 ? p.t_max : 0;
    } else if (c->diffusion_type == DSD_DIFFUSE_REFLOW) {
        if (source) {
            const float a = 1.0f - depth, b = c->t_start;       // torch.maximum(1 - depth, T_start) on fp32 tensors
            p.t_start = a > b ? a : b;
            if (p.t_start >= 1.f) {
                p.start = DSD_AC_START_SOURCE;
                p.src_scale = 1.f;
                p.noise_scale = 0.f;
            } else if (p.t_start > 0.f) {
                p.start = DSD_AC_START_MIX;
                p.src_scale = p.t_start;
                p.noise_scale = (float)(1.0 - (double)p.t_start);
            }
        }
    } else {
        return fail(nullptr, DSD_EINVAL, "%s: diffusion_type = %d", who, c->diffusion_type);
    }
    *out = p;
    return DSD_OK;
}
