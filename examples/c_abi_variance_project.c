/*
 * A variance project from ONE model file in plain C: three segments with different phone, word, note and frame counts go
 * through the variance model as one padded, ragged, per-item-seeded batch - score in; durations, pitch and curves out.  No
 * Python, no torch, and no constant of the model in this source: only include/dsdenoise.h and the HIP runtime for device
 * memory.  The model file is what examples/pack_model.py --variance packs: the word form (predict_dur) with both predictors,
 * rectified flow.  The steps, each one library call:
 *
 *   1. dsd_seconds_to_frames        the notes' seconds -> frames; a segment's frame count is their total (host arithmetic)
 *   2. dsd_word_dur                 word durations from the note slurs, aligned to those totals
 *   3. dsd_variance_encode          the linguistic encoder on the words' durations; it also gives ph2word ...
 *      dsd_group_midi               ... through which the words' mean MIDI becomes the phones' `midi` input
 *   4. dsd_variance_spk_mix         the speaker mix, where the file has speakers
 *   5. dsd_variance_dur             predicted phone durations
 *   6. dsd_rhythm_align             ... scaled to the words and rounded: the integer durations every later stage takes
 *   7. dsd_variance_set_lengths     the segments' frame counts, for the stages and both denoisers
 *   8. dsd_variance_pitch_cond, x_T from dsd_noise_fill under one seed per segment, dsd_sample, dsd_variance_pitch_post
 *   9. dsd_variance_cond on the predicted pitch, dsd_sample, dsd_variance_post
 *
 * Every segment comes out as if it had been rendered alone.  Prints one figure per stage and segment over the segment's own
 * phones or frames (`sum <name> <segment> <value>`); tests/test_gpu_words.py compiles this with gcc, runs it on the MI355X
 * and compares the figures with the same chain driven from Python, and each segment with its lone render.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_variance_project.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o variance_project
 *   ./variance_project model.dsdm var
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsdenoise.h"

#define CHECK(handle, call)                                                                  \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0) {                                                                      \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dsd_last_error(handle));     \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

/* the project: three segments, padded to the largest of each count */
enum { B = 3, L = 6, W = 3, N = 5, T_MAX = 512, STEPS = 4 };
static const int n_ph[B] = {6, 3, 5}, n_word[B] = {3, 1, 2}, n_note[B] = {5, 2, 4};
static const int64_t word_div[B][W] = {{2, 1, 3}, {3, 0, 0}, {2, 3, 0}};                       /* phones per word */
static const float note_seconds[B][N] = {{0.21f, 0.17f, 0.30f, 0.12f, 0.26f}, {0.25f, 0.19f}, {0.15f, 0.22f, 0.11f, 0.33f}};
static const uint8_t note_slur[B][N] = {{0, 1, 0, 0, 1}, {0, 1, 1, 1, 1}, {0, 0, 1, 1, 1}};    /* padding notes: slur 1 */
static const float note_pitch[B][N] = {{60.0f, 62.0f, 64.5f, 59.0f, 57.0f}, {67.0f, 65.5f, -1.f, -1.f, -1.f}, {55.0f, 58.0f, 60.0f, 62.0f, -1.f}};
static const uint64_t seeds[B] = {2025, 2026, 2027};
static const double TIMESTEP = 512.0 / 44100.0;                 /* the project's hop: the caller's, not the model's */
enum { DOMAIN_PITCH_X_T = 6, DOMAIN_VARIANCE_X_T = 7 };        /* the Python side's domains (dsd_noise_fill) */

static int32_t lens[B];         /* the segments' frame counts */
static int T;                   /* the largest of them: the padded batch's frames */

static void* to_device(const void* src, size_t bytes) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    if (src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
    if (!src && hipMemset(d, 0, bytes) != hipSuccess) return NULL;
    return d;
}

/* one figure per segment: the sum over its own `valid[b]` rows of `width` values, out of `rows` padded rows */
static int print_sums(const char* name, const void* dev, int is_int, int rows, const int* valid, int width) {
    const size_t n = (size_t)B * rows * width, size = is_int ? sizeof(int64_t) : sizeof(float);
    void* host = malloc(n * size);
    if (!host || hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, dev, n * size, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    for (int b = 0; b < B; ++b) {
        double sum = 0.0;
        for (size_t i = 0; i < (size_t)valid[b] * width; ++i) {
            const size_t at = (size_t)b * rows * width + i;
            sum += is_int ? (double)((const int64_t*)host)[at] : (double)((const float*)host)[at];
        }
        printf("sum %s %d %.17g\n", name, b, sum);
    }
    free(host);
    return 0;
}

/* the sampler stage: x_T under one seed per segment, the condition, the loop; out is [B, F, T, M] denormalised */
static int sample(dsd_handle* h, const dsd_program* prog, uint32_t domain, const float* cond, int H, int F, int M, const float* lo,
                  const float* hi, float* out) {
    float scale[DSD_VAR_MAX_CURVES * 256], shift[DSD_VAR_MAX_CURVES * 256];
    if (M > 256) return 1;
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < M; ++m) {
            scale[f * M + m] = (hi[f] - lo[f]) / 2.0f;        /* the twins' x * k + b */
            shift[f * M + m] = (hi[f] + lo[f]) / 2.0f;
        }
    float* d_scale = (float*)to_device(scale, sizeof(float) * (size_t)(F * M));
    float* d_shift = (float*)to_device(shift, sizeof(float) * (size_t)(F * M));
    float* x_t = (float*)to_device(NULL, sizeof(float) * (size_t)B * F * M * T);
    if (!d_scale || !d_shift || !x_t) return 1;
    dsd_noise_spec ns;
    memset(&ns, 0, sizeof(ns));
    ns.struct_size = (int32_t)sizeof(ns);
    ns.kind = DSD_NOISE_NORMAL;
    ns.domain = domain;
    ns.n = 1; ns.B = B; ns.rows = F * M; ns.cols = T;
    ns.seeds = seeds;               /* element (row, t) of a segment's x_T does not depend on T: the lone render draws the same */
    ns.scale = 1.0f;
    CHECK(NULL, dsd_noise_fill(0, &ns, x_t, NULL));
    CHECK(h, dsd_prepare_cond(h, cond, B, T, (int64_t)T * H, 1, H, NULL));        /* cond is [B, T, H] */
    CHECK(h, dsd_sample(h, prog, x_t, NULL, out, d_scale, d_shift, DSD_SAMPLE_TRANSPOSE, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    (void)hipFree(d_scale);
    (void)hipFree(d_shift);
    (void)hipFree(x_t);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s model.dsdm prefix\n", argv[0]);
        return 2;
    }
    dsd_model_file* mf = NULL;
    CHECK(NULL, dsd_model_open(argv[1], &mf));
    dsd_variance* v = NULL;
    CHECK(NULL, dsd_variance_open(mf, argv[2], /*device=*/0, &v));
    dsd_model_close(mf);            /* the object holds its own copies */
    dsd_variance_config c;
    CHECK(NULL, dsd_variance_info(v, &c));
    const int H = c.hidden_size;
    int n_var = 0, slot[DSD_VAR_MAX_CURVES];
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i)
        if ((c.variances >> i) & 1u) slot[n_var++] = i;
    static const char* const names[DSD_VAR_MAX_CURVES] = {"energy", "breathiness", "voicing", "tension"};
    if (!c.predict_dur || !c.predict_pitch || !n_var || c.diffusion_type != DSD_DIFFUSE_REFLOW) {
        fprintf(stderr, "this example drives a word-form model with rectified-flow pitch and variance predictors\n");
        return 1;
    }

    /* 1. the notes' frames; a segment's frame count is its notes' total */
    int64_t note_dur[B][N], totals[B];
    memset(note_dur, 0, sizeof(note_dur));
    T = 0;
    for (int b = 0; b < B; ++b) {
        CHECK(NULL, dsd_seconds_to_frames(note_seconds[b], n_note[b], TIMESTEP, note_dur[b], &totals[b]));
        if (totals[b] > T_MAX) return 3;
        lens[b] = (int32_t)totals[b];
        if (lens[b] > T) T = lens[b];
    }
    printf("api v%d  hidden %d  %d segments of %d, %d and %d frames in a batch of %d\n", dsd_api_version(), H, B, (int)lens[0], (int)lens[1],
           (int)lens[2], T);

    /* what an editor has besides: tokens, languages, rests, glides, the speakers */
    int64_t tokens[B][L], languages[B][L], note_glide[B][N];
    uint8_t note_rest[B][N];
    memset(tokens, 0, sizeof(tokens));                          /* token 0: a padding phone */
    memset(languages, 0, sizeof(languages));
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < n_ph[b]; ++i) {
            tokens[b][i] = 1 + (3 * i + 5 * b) % (c.vocab_size - 1);
            languages[b][i] = c.num_lang > 0 ? 1 + (i + b) % c.num_lang : 0;
        }
        for (int k = 0; k < N; ++k) {
            note_glide[b][k] = (c.glide_rows > 0 && k < n_note[b]) ? (k + b) % c.glide_rows : 0;
            note_rest[b][k] = (uint8_t)(k < n_note[b] && (k + b) % 4 == 3);
        }
    }
    const size_t bt = (size_t)B * T;
    float* pitch = (float*)malloc(sizeof(float) * bt);
    float* spk_w = (float*)malloc(sizeof(float) * (size_t)B * 2);
    if (!pitch || !spk_w) return 3;
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < T; ++t) pitch[(size_t)b * T + t] = 60.0f + 0.03125f * (float)((t + 7 * b) % 96);      /* past a segment's end: junk */
        spk_w[2 * b] = 0.25f * (float)(b + 1);
        spk_w[2 * b + 1] = 1.0f - spk_w[2 * b];
    }
    const int32_t spk_ids[B * 2] = {0, c.num_spk > 1 ? 1 : 0, 0, c.num_spk > 1 ? 1 : 0, 0, c.num_spk > 1 ? 1 : 0};

    int64_t* d_tokens = (int64_t*)to_device(tokens, sizeof(tokens));
    int64_t* d_languages = (int64_t*)to_device(languages, sizeof(languages));
    int64_t* d_word_div = (int64_t*)to_device(word_div, sizeof(word_div));
    int64_t* d_note_dur = (int64_t*)to_device(note_dur, sizeof(note_dur));
    int64_t* d_note_glide = (int64_t*)to_device(note_glide, sizeof(note_glide));
    uint8_t* d_note_slur = (uint8_t*)to_device(note_slur, sizeof(note_slur));
    uint8_t* d_note_rest = (uint8_t*)to_device(note_rest, sizeof(note_rest));
    float* d_note_midi = (float*)to_device(note_pitch, sizeof(note_pitch));
    float* d_pitch = (float*)to_device(pitch, sizeof(float) * bt);
    float* d_spk_w = (float*)to_device(spk_w, sizeof(float) * (size_t)B * 2);
    int64_t* d_word_dur = (int64_t*)to_device(NULL, sizeof(int64_t) * B * W);
    int64_t* d_ph2word = (int64_t*)to_device(NULL, sizeof(int64_t) * B * L);
    int64_t* d_ph_midi = (int64_t*)to_device(NULL, sizeof(int64_t) * B * L);
    int64_t* d_ph_dur = (int64_t*)to_device(NULL, sizeof(int64_t) * B * L);
    float* d_spk = c.use_spk_id ? (float*)to_device(NULL, sizeof(float) * (size_t)B * H) : NULL;
    float* d_enc = (float*)to_device(NULL, sizeof(float) * (size_t)B * L * H);
    uint8_t* d_masks = (uint8_t*)to_device(NULL, (size_t)B * L);
    float* d_dur = (float*)to_device(NULL, sizeof(float) * (size_t)B * L);
    float* d_cond = (float*)to_device(NULL, sizeof(float) * bt * H);
    float* d_base = (float*)to_device(NULL, sizeof(float) * bt);
    float* d_pred = (float*)to_device(NULL, sizeof(float) * bt);
    float* d_raw = (float*)to_device(NULL, sizeof(float) * bt * (size_t)c.pitch_repeat_bins);
    uint8_t* d_all_true = (uint8_t*)to_device(NULL, bt * DSD_VAR_MAX_CURVES);
    if (!d_tokens || !d_languages || !d_word_div || !d_note_dur || !d_note_glide || !d_note_slur || !d_note_rest || !d_note_midi || !d_pitch ||
        !d_spk_w || !d_word_dur || !d_ph2word || !d_ph_midi || !d_ph_dur || (c.use_spk_id && !d_spk) || !d_enc || !d_masks || !d_dur || !d_cond ||
        !d_base || !d_pred || !d_raw || !d_all_true || hipMemset(d_all_true, 1, bt * DSD_VAR_MAX_CURVES) != hipSuccess)
        return 3;

    /* 2. word durations from the slurs, aligned to the segments' frame counts */
    dsd_word_dur_args wa;
    memset(&wa, 0, sizeof(wa));
    wa.struct_size = (int32_t)sizeof(wa);
    wa.B = B; wa.N = N; wa.W = W;
    wa.dur = d_note_dur; wa.slur = d_note_slur; wa.totals = totals; wa.word_dur = d_word_dur;
    CHECK(NULL, dsd_word_dur(0, &wa, NULL));
    if (print_sums("word_dur", d_word_dur, 1, W, n_word, 1)) return 3;

    /* 3. the linguistic encoder, word form; its ph2word gathers the words' mean MIDI to the phones */
    dsd_variance_encode_args ea;
    memset(&ea, 0, sizeof(ea));
    ea.struct_size = (int32_t)sizeof(ea);
    ea.B = B; ea.L = L; ea.W = W;
    ea.tokens = d_tokens; ea.word_div = d_word_div; ea.word_dur = d_word_dur; ea.languages = d_languages;
    ea.encoder_out = d_enc; ea.x_masks = d_masks; ea.ph2word = d_ph2word;
    CHECK(NULL, dsd_variance_encode(v, &ea, NULL));
    if (print_sums("encoder_out", d_enc, 0, L, n_ph, H)) return 3;
    dsd_group_midi_args ga;
    memset(&ga, 0, sizeof(ga));
    ga.struct_size = (int32_t)sizeof(ga);
    ga.B = B; ga.Nn = N; ga.G = W; ga.L = L; ga.T = T;
    ga.note_midi = d_note_midi; ga.note_dur = d_note_dur; ga.group_dur = d_word_dur; ga.ph2word = d_ph2word; ga.midi = d_ph_midi;
    CHECK(NULL, dsd_group_midi(0, &ga, NULL));
    if (print_sums("ph_midi", d_ph_midi, 1, L, n_ph, 1)) return 3;

    /* 4. one speaker mix per segment */
    if (d_spk) {
        dsd_spk_mix_args ma;
        memset(&ma, 0, sizeof(ma));
        ma.struct_size = (int32_t)sizeof(ma);
        ma.B = B; ma.rows = 1; ma.N = 2;
        ma.ids = spk_ids; ma.values = d_spk_w; ma.out = d_spk;
        CHECK(NULL, dsd_variance_spk_mix(v, &ma, NULL));
    }

    /* 5. predicted phone durations, 6. scaled to the words and rounded */
    dsd_variance_dur_args da;
    memset(&da, 0, sizeof(da));
    da.struct_size = (int32_t)sizeof(da);
    da.B = B; da.L = L;
    da.encoder_out = d_enc; da.x_masks = d_masks; da.ph_midi = d_ph_midi; da.spk_embed = d_spk; da.spk_rows = d_spk ? 1 : 0;
    da.ph_dur_pred = d_dur;
    CHECK(NULL, dsd_variance_dur(v, &da, NULL));
    if (print_sums("ph_dur_pred", d_dur, 0, L, n_ph, 1)) return 3;
    dsd_rhythm_align_args ra;
    memset(&ra, 0, sizeof(ra));
    ra.struct_size = (int32_t)sizeof(ra);
    ra.B = B; ra.L = L; ra.W = W;
    ra.ph_dur_pred = d_dur; ra.ph2word = d_ph2word; ra.word_dur = d_word_dur; ra.ph_dur = d_ph_dur;
    CHECK(NULL, dsd_rhythm_align(0, &ra, NULL));
    if (print_sums("ph_dur", d_ph_dur, 1, L, n_ph, 1)) return 3;

    /* 7. the segments' frame counts: the stages below and both denoisers */
    CHECK(NULL, dsd_variance_set_lengths(v, lens, B, NULL));
    int frames[B];
    for (int b = 0; b < B; ++b) frames[b] = lens[b];

    /* 8. the pitch: condition (every frame retaken), x_T, the rectified-flow loop, the curve */
    dsd_variance_pitch_cond_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.struct_size = (int32_t)sizeof(pa);
    pa.B = B; pa.L = L; pa.N = N; pa.T = T;
    pa.encoder_out = d_enc; pa.ph_dur = d_ph_dur; pa.note_midi = d_note_midi; pa.note_rest = d_note_rest; pa.note_dur = d_note_dur;
    pa.note_glide = c.use_glide_embed ? d_note_glide : NULL;
    pa.pitch = d_pitch; pa.retake = d_all_true; pa.spk_embed = d_spk; pa.spk_rows = d_spk ? 1 : 0;
    pa.pitch_cond = d_cond; pa.base_pitch = d_base;         /* lengths NULL: the object's own */
    CHECK(NULL, dsd_variance_pitch_cond(v, &pa, NULL));
    if (print_sums("pitch_cond", d_cond, 0, T, frames, H) || print_sums("base_pitch", d_base, 0, T, frames, 1)) return 3;
    dsd_sampler_spec ss;
    memset(&ss, 0, sizeof(ss));
    ss.struct_size = (int32_t)sizeof(ss);
    ss.sampler = DSD_SAMPLER_RF_EULER_ONNX;
    ss.steps = STEPS;
    ss.t_start = 0.0;
    ss.time_scale_factor = c.time_scale_factor;
    dsd_program* prog = NULL;
    CHECK(NULL, dsd_program_build(&ss, &prog));
    dsd_handle* pitch_net = NULL;
    CHECK(NULL, dsd_variance_backbone(v, DSD_VAR_PITCH, &pitch_net));
    if (sample(pitch_net, prog, DOMAIN_PITCH_X_T, d_cond, H, 1, c.pitch_repeat_bins, &c.pitd_norm_min, &c.pitd_norm_max, d_raw)) return 1;
    CHECK(NULL, dsd_variance_pitch_post(v, d_raw, d_base, B, T, d_pred, NULL));
    if (print_sums("pitch_pred", d_pred, 0, T, frames, 1)) return 3;

    /* 9. the curves: condition on the predicted pitch (every variance retaken), the loop, the curves */
    float* d_zero = (float*)to_device(NULL, sizeof(float) * bt);
    float* d_vcond = (float*)to_device(NULL, sizeof(float) * bt * H);
    float* d_vraw = (float*)to_device(NULL, sizeof(float) * bt * n_var * (size_t)c.var_repeat_bins);
    float* d_curves[DSD_VAR_MAX_CURVES] = {NULL, NULL, NULL, NULL};
    if (!d_zero || !d_vcond || !d_vraw) return 3;
    dsd_variance_cond_args ca;
    memset(&ca, 0, sizeof(ca));
    ca.struct_size = (int32_t)sizeof(ca);
    ca.B = B; ca.L = L; ca.T = T;
    ca.encoder_out = d_enc; ca.ph_dur = d_ph_dur; ca.pitch = d_pred; ca.retake = d_all_true;
    ca.spk_embed = d_spk; ca.spk_rows = d_spk ? 1 : 0; ca.variance_cond = d_vcond;
    float lo[DSD_VAR_MAX_CURVES], hi[DSD_VAR_MAX_CURVES];
    for (int i = 0; i < n_var; ++i) {
        ca.curves[i] = d_zero;
        lo[i] = c.var_norm_min[slot[i]];
        hi[i] = c.var_norm_max[slot[i]];
        d_curves[i] = (float*)to_device(NULL, sizeof(float) * bt);
        if (!d_curves[i]) return 3;
    }
    CHECK(NULL, dsd_variance_cond(v, &ca, NULL));
    if (print_sums("variance_cond", d_vcond, 0, T, frames, H)) return 3;
    dsd_handle* var_net = NULL;
    CHECK(NULL, dsd_variance_backbone(v, DSD_VAR_VARIANCES, &var_net));
    if (sample(var_net, prog, DOMAIN_VARIANCE_X_T, d_vcond, H, n_var, c.var_repeat_bins, lo, hi, d_vraw)) return 1;
    CHECK(NULL, dsd_variance_post(v, d_vraw, B, T, d_curves, NULL));
    for (int i = 0; i < n_var; ++i)
        if (print_sums(names[slot[i]], d_curves[i], 0, T, frames, 1)) return 3;

    dsd_program_free(prog);
    dsd_variance_close(v);      /* releases the borrowed handles too */
    free(pitch);
    free(spk_w);
    return 0;
}
