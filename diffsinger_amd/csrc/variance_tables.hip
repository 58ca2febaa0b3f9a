// libdsdenoise, the host-only half of dsd_variance_open: what a DSD_VARIANCE_TABLES section must hold for its config, what
// the inner sections' configs must say, and the smoothing taps.  No kernel, no HIP call, no HIP header - like
// model_file.hip, so tools/harness/variance_harness.cpp compiles this file with a plain host compiler under the sanitizers.
// Everything is checked here before dsd_variance_open touches a device (variance_api.hip).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "variance_tables.h"

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);

const char* const kVarianceNames[DSD_VAR_MAX_CURVES] = {"energy", "breathiness", "voicing", "tension"};

namespace {

const char* const WHO = "dsd_variance_open";

struct Want {
    char name[96];
    int64_t shape[2];
    int ndim;
    bool required;      // false: the flags exclude it
    bool optional;      // with required: may be absent
    int* slot;
};

int find(const dsd_model_tensor_info* t, int32_t n, const char* name) {
    for (int32_t j = 0; j < n; ++j)
        if (t[j].name && strcmp(t[j].name, name) == 0) return j;
    return -1;
}

bool is_flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace

int variance_tables_check(const dsd_variance_config* c, int32_t cfg_size, const dsd_model_tensor_info* tensors, int32_t n_tensors,
                          const char* section, VarianceTableIndex* index) {
    if (!c || !section || !index || (n_tensors > 0 && !tensors)) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
    if (cfg_size != (int32_t)sizeof(dsd_variance_config) || c->struct_size != (int32_t)sizeof(dsd_variance_config))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": struct_size %d (config of %d bytes) != %zu", WHO, section,
                    cfg_size == (int32_t)sizeof(dsd_variance_config) ? c->struct_size : -1, cfg_size, sizeof(dsd_variance_config));
    const struct { const char* name; int32_t v; } flags[] = {
        {"predict_dur", c->predict_dur}, {"predict_pitch", c->predict_pitch}, {"use_melody_encoder", c->use_melody_encoder},
        {"use_glide_embed", c->use_glide_embed}, {"use_lang_id", c->use_lang_id}, {"use_spk_id", c->use_spk_id}};
    for (const auto& f : flags)
        if (!is_flag(f.v)) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": %s = %d is neither 0 nor 1", WHO, section, f.name, f.v);
    if (c->hidden_size < 1 || c->vocab_size < 1)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": hidden_size %d and vocab_size %d must be positive", WHO, section, c->hidden_size,
                    c->vocab_size);
    if (c->variances >= (1u << DSD_VAR_MAX_CURVES))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": variances = 0x%x has a bit above DSD_EMBED_TENSION", WHO, section, c->variances);
    if (c->use_melody_encoder && !c->predict_pitch)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_melody_encoder without predict_pitch", WHO, section);
    if (c->use_glide_embed && !c->use_melody_encoder)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_glide_embed without use_melody_encoder", WHO, section);
    if (c->use_lang_id && c->num_lang < 1) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_lang_id with num_lang = %d", WHO, section, c->num_lang);
    if (c->use_spk_id && c->num_spk < 1) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": use_spk_id with num_spk = %d", WHO, section, c->num_spk);
    if (c->use_melody_encoder && c->melody_hidden_size < 1)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": melody_hidden_size = %d with a melody encoder", WHO, section, c->melody_hidden_size);
    if (c->use_glide_embed && c->glide_rows < 1) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": glide_rows = %d with a glide table", WHO, section, c->glide_rows);
    if (c->predict_pitch) {
        if (c->smooth_width < 1 || c->smooth_width > 255)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": smooth_width K = %d outside [1, 255]", WHO, section, c->smooth_width);
        if (c->pitch_repeat_bins < 1) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": pitch_repeat_bins = %d", WHO, section, c->pitch_repeat_bins);
    }
    if (c->variances && c->var_repeat_bins < 1) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": var_repeat_bins = %d", WHO, section, c->var_repeat_bins);
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i)
        if (!is_flag(c->var_no_clamp[i])) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": var_no_clamp[%d] = %d is neither 0 nor 1", WHO, section, i, c->var_no_clamp[i]);
    if (c->diffusion_type != DSD_DIFFUSE_DDPM && c->diffusion_type != DSD_DIFFUSE_REFLOW)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": diffusion_type = %d", WHO, section, c->diffusion_type);

    VarianceTableIndex& ix = *index;
    memset(&ix, 0xFF, sizeof(ix));          // every slot -1
    ix.mask_any = 0;
    const int64_t H = c->hidden_size, Hm = c->melody_hidden_size;
    const bool dur = c->predict_dur, pit = c->predict_pitch, mel = c->use_melody_encoder, var = c->variances != 0;
    Want want[40];
    int nw = 0;
    auto add = [&](const char* name, int64_t d0, int64_t d1, bool required, int* slot) {
        Want& w = want[nw++];
        snprintf(w.name, sizeof(w.name), "%s", name);
        w.shape[0] = d0; w.shape[1] = d1; w.ndim = d1 < 0 ? 1 : 2; w.required = required; w.optional = false; w.slot = slot;
    };
    auto lin1 = [&](const char* prefix, int64_t h, bool required, int* w_slot, int* b_slot) {
        char name[96];
        snprintf(name, sizeof(name), "%s.weight", prefix);
        add(name, h, 1, required, w_slot);
        snprintf(name, sizeof(name), "%s.bias", prefix);
        add(name, h, -1, required, b_slot);
    };
    add("fs2.txt_embed.weight", c->vocab_size, H, true, &ix.txt);
    add("cross_lingual_mask", c->vocab_size, -1, true, &ix.mask);
    add("fs2.lang_embed.weight", (int64_t)c->num_lang + 1, H, c->use_lang_id, &ix.lang);
    add("fs2.onset_embed.weight", 2, H, dur, &ix.onset);
    int other_w = -1, other_b = -1;
    lin1("fs2.word_dur_embed", H, dur, dur ? &ix.dur_w : &other_w, dur ? &ix.dur_b : &other_b);
    lin1("fs2.ph_dur_embed", H, !dur, dur ? &other_w : &ix.dur_w, dur ? &other_b : &ix.dur_b);
    add("fs2.midi_embed.weight", 128, H, dur, &ix.midi);
    add("spk_embed.weight", c->num_spk, H, c->use_spk_id, &ix.spk);
    lin1("melody_encoder.note_midi_embed", Hm, mel, &ix.note_midi_w, &ix.note_midi_b);
    lin1("melody_encoder.note_dur_embed", Hm, mel, &ix.note_dur_w, &ix.note_dur_b);
    add("melody_encoder.note_glide_embed.weight", c->glide_rows, Hm, c->use_glide_embed, &ix.glide);
    add("pitch_retake_embed.weight", 2, H, pit, &ix.retake);
    lin1("delta_pitch_embed", H, pit && mel, mel ? &ix.pitch_in_w : &other_w, mel ? &ix.pitch_in_b : &other_b);
    lin1("base_pitch_embed", H, pit && !mel, mel ? &other_w : &ix.pitch_in_w, mel ? &other_b : &ix.pitch_in_b);
    add("smooth_taps", c->smooth_width, -1, pit, &ix.taps);        // the exporter's own taps, if it stored them
    want[nw - 1].optional = true;
    lin1("pitch_embed", H, var, &ix.pitch_w, &ix.pitch_b);
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i) {
        char prefix[64];
        snprintf(prefix, sizeof(prefix), "variance_embeds.%s", kVarianceNames[i]);
        lin1(prefix, H, (c->variances >> i) & 1u, &ix.var_w[i], &ix.var_b[i]);
    }

    int matched = 0;
    for (int k = 0; k < nw; ++k) {
        const Want& w = want[k];
        const int j = find(tensors, n_tensors, w.name);
        if (j < 0) {
            if (w.required && !w.optional) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" lacks the tensor \"%s\" its config requires", WHO, section, w.name);
            continue;
        }
        if (!w.required) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" carries the tensor \"%s\", which its config excludes", WHO, section, w.name);
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
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" carries the tensor \"%s\", which the variance model's tables do not have", WHO,
                            section, tensors[j].name ? tensors[j].name : "(null)");
        }
    if (ix.taps >= 0 && c->smooth_width >= 2) {       // stored taps decide the smoothing: finite, and a weighted mean (K = 1 is the
        const float* w = tensors[ix.taps].data;       // reference's 0 / 0 and is taken as stored)
        double sum = 0.0;
        for (int k = 0; k < c->smooth_width; ++k) {
            if (!isfinite(w[k])) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": smooth_taps[%d] is not finite", WHO, section, k);
            sum += (double)w[k];
        }
        if (fabs(sum - 1.0) > 1e-4)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": smooth_taps sum to %.9g, not to 1 (within 1e-4)", WHO, section, sum);
    }
    const float* mask = tensors[ix.mask].data;
    for (int64_t i = 0; i < c->vocab_size; ++i) {
        if (mask[i] != 0.f && mask[i] != 1.f)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": cross_lingual_mask[%lld] = %g is neither 0 nor 1", WHO, section, (long long)i, (double)mask[i]);
        if (mask[i] == 1.f) ix.mask_any = 1;
    }
    return DSD_OK;
}

int variance_inner_check(const dsd_variance_config* c, const dsd_token_encoder_config* fs2, const dsd_token_encoder_config* melody,
                         const dsd_config* pitch, const dsd_config* variances) {
    if (!c || !fs2) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
#define SAME(have, want, lhs, rhs)                                                                                           \
    if ((have) != (want)) return fail(nullptr, DSD_EINVAL, "%s: " lhs " = %d does not match " rhs " = %d", WHO, (int)(have), (int)(want))
    SAME(fs2->hidden_size, c->hidden_size, "fs2.hidden_size", "tables.hidden_size");
    SAME(fs2->out_dims, 0, "fs2.out_dims", "the encoder's own width, out_dims");
    if ((fs2->dur_layers > 0) != (c->predict_dur != 0))
        return fail(nullptr, DSD_EINVAL, "%s: fs2.dur_layers = %d does not match tables.predict_dur = %d", WHO, fs2->dur_layers, c->predict_dur);
    if (c->use_melody_encoder) {
        if (!melody) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
        SAME(melody->hidden_size, c->melody_hidden_size, "melody.hidden_size", "tables.melody_hidden_size");
        SAME(melody->out_dims, c->hidden_size, "melody.out_dims", "tables.hidden_size");
        SAME(melody->dur_layers, 0, "melody.dur_layers", "a melody encoder's dur_layers");
    }
    if (c->predict_pitch) {
        if (!pitch) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
        SAME(pitch->hidden_size, c->hidden_size, "pitch.hidden_size", "tables.hidden_size");
        SAME(pitch->in_dims, c->pitch_repeat_bins, "pitch.in_dims", "tables.pitch_repeat_bins");
        SAME(pitch->n_feats, 1, "pitch.n_feats", "the one curve of a pitch predictor, n_feats");
    }
    if (c->variances) {
        if (!variances) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
        SAME(variances->hidden_size, c->hidden_size, "variances.hidden_size", "tables.hidden_size");
        SAME(variances->in_dims, c->var_repeat_bins, "variances.in_dims", "tables.var_repeat_bins");
        SAME(variances->n_feats, variance_count(c->variances), "variances.n_feats", "the bits set in tables.variances,");
    }
#undef SAME
    return DSD_OK;
}

void variance_smooth_taps(int K, float* w) {
    // np.linspace(0, 1, K) in double (i * step, the last point exactly 1), rounded to fp32, times fp32 pi; the sine of that
    // fp32 argument rounded from double; the sum added in double and rounded once; an fp32 division.  K = 1: 0 / 0.
    const double step = K > 1 ? 1.0 / (double)(K - 1) : 0.0;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const float x = (float)(K > 1 && k == K - 1 ? 1.0 : (double)k * step);
        const float arg = x * (float)M_PI;
        w[k] = (float)sin((double)arg);
        sum += (double)w[k];
    }
    const float total = (float)sum;
    for (int k = 0; k < K; ++k) w[k] = w[k] / total;
}

}  // namespace dsd
