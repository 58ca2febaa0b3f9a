/*
 * The variance model's staged twin from ONE model file in plain C: no Python, no torch, and no constant of the model in
 * this source - only include/dsdenoise.h and the HIP runtime for device memory.  Opens the file
 * (examples/pack_model.py --variance packs one), opens the variance object under a prefix (dsd_variance_open), reads every
 * size and range from dsd_variance_info, and runs a small synthetic segment through the stages an editor drives:
 *
 *   dsd_variance_encode (word form) -> dsd_variance_dur -> dsd_variance_pitch_cond
 *   -> dsd_program_build (the twin's rectified-flow euler loop) + dsd_noise_fill (x_T) + dsd_prepare_cond + dsd_sample on
 *      the handle dsd_variance_backbone lends out -> dsd_variance_pitch_post
 *   -> dsd_variance_cond on the predicted pitch -> the same sampler stage on the variance predictor -> dsd_variance_post
 *
 * and prints the sum of every stage's output (`sum <name> <value>`).  tests/test_gpu_cvariance.py compiles this with gcc,
 * runs it on the MI355X and compares the sums with the same chain driven from Python on the same file, inputs and seed.
 * The model must be of the word form (predict_dur) with a rectified-flow pitch predictor; the variance half runs when
 * the model predicts variances.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_variance.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o variance_demo
 *   ./variance_demo model.dsdm var
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

/* the segment: sizes and seed are the caller's, not the model's */
enum { B = 1, L = 6, W = 3, N = 4, T = 120, STEPS = 4 };
static const uint64_t SEED = 2025;
enum { DOMAIN_PITCH_X_T = 6, DOMAIN_VARIANCE_X_T = 7 };        /* the Python side's domains (dsd_noise_fill) */

static void* to_device(const void* src, size_t bytes) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    if (src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
    if (!src && hipMemset(d, 0, bytes) != hipSuccess) return NULL;
    return d;
}

static int print_sum(const char* name, const float* dev, size_t n) {
    float* host = (float*)malloc(n * sizeof(float));
    if (!host || hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) sum += (double)host[i];
    printf("sum %s %.17g\n", name, sum);
    free(host);
    return 0;
}

/* the sampler stage: x_T under the seed, the condition, the loop; out is [B, F, T, M] denormalised by scale / shift */
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
    ns.seeds = &SEED;
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
    printf("api v%d  hidden %d  vocab %d  K %d  pitch bins %d  %d variances x %d bins\n", dsd_api_version(), H, (int)c.vocab_size,
           (int)c.smooth_width, (int)c.pitch_repeat_bins, n_var, (int)c.var_repeat_bins);
    if (!c.predict_dur || !c.predict_pitch || c.diffusion_type != DSD_DIFFUSE_REFLOW) {
        fprintf(stderr, "this example drives a word-form model with a rectified-flow pitch predictor\n");
        return 1;
    }

    /* the inputs an editor would have: tokens, words, notes, curves */
    int64_t tokens[L], languages[L], ph_midi[L], note_glide[N];
    for (int i = 0; i < L; ++i) {
        tokens[i] = 1 + (3 * i) % (c.vocab_size - 1);
        languages[i] = c.num_lang > 0 ? 1 + i % c.num_lang : 0;
        ph_midi[i] = 60 + i;
    }
    const int64_t word_div[W] = {2, 1, 3}, word_dur[W] = {50, 30, 40};
    const int64_t ph_dur[L] = {25, 25, 30, 10, 0, 30}, note_dur[N] = {30, 30, 20, 40};
    const float note_midi[N] = {60.0f, 62.5f, 64.0f, 59.0f};
    const uint8_t note_rest[N] = {0, 0, 1, 0};
    for (int k = 0; k < N; ++k) note_glide[k] = c.glide_rows > 0 ? k % c.glide_rows : 0;
    float pitch[T];
    uint8_t retake[T], all_true[T * DSD_VAR_MAX_CURVES];
    for (int t = 0; t < T; ++t) {
        pitch[t] = 60.0f + 0.03125f * (float)t;
        retake[t] = (uint8_t)((t / 16) % 2 == 0);
    }
    memset(all_true, 1, sizeof(all_true));
    float* spk = (float*)malloc(sizeof(float) * (size_t)H);
    if (!spk) return 3;
    for (int h = 0; h < H; ++h) spk[h] = 0.015625f * (float)(h % 7 - 3);

    int64_t* d_tokens = (int64_t*)to_device(tokens, sizeof(tokens));
    int64_t* d_languages = (int64_t*)to_device(languages, sizeof(languages));
    int64_t* d_ph_midi = (int64_t*)to_device(ph_midi, sizeof(ph_midi));
    int64_t* d_word_div = (int64_t*)to_device(word_div, sizeof(word_div));
    int64_t* d_word_dur = (int64_t*)to_device(word_dur, sizeof(word_dur));
    int64_t* d_ph_dur = (int64_t*)to_device(ph_dur, sizeof(ph_dur));
    int64_t* d_note_dur = (int64_t*)to_device(note_dur, sizeof(note_dur));
    int64_t* d_note_glide = (int64_t*)to_device(note_glide, sizeof(note_glide));
    float* d_note_midi = (float*)to_device(note_midi, sizeof(note_midi));
    uint8_t* d_note_rest = (uint8_t*)to_device(note_rest, sizeof(note_rest));
    float* d_pitch = (float*)to_device(pitch, sizeof(pitch));
    uint8_t* d_retake = (uint8_t*)to_device(retake, sizeof(retake));
    uint8_t* d_all_true = (uint8_t*)to_device(all_true, sizeof(all_true));
    float* d_spk = c.use_spk_id ? (float*)to_device(spk, sizeof(float) * (size_t)H) : NULL;
    float* d_enc = (float*)to_device(NULL, sizeof(float) * (size_t)B * L * H);
    uint8_t* d_masks = (uint8_t*)to_device(NULL, (size_t)B * L);
    float* d_dur = (float*)to_device(NULL, sizeof(float) * (size_t)B * L);
    float* d_cond = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * H);
    float* d_base = (float*)to_device(NULL, sizeof(float) * (size_t)B * T);
    float* d_pred = (float*)to_device(NULL, sizeof(float) * (size_t)B * T);
    float* d_raw = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * (size_t)c.pitch_repeat_bins);
    if (!d_tokens || !d_languages || !d_ph_midi || !d_word_div || !d_word_dur || !d_ph_dur || !d_note_dur || !d_note_glide || !d_note_midi ||
        !d_note_rest || !d_pitch || !d_retake || !d_all_true || (c.use_spk_id && !d_spk) || !d_enc || !d_masks || !d_dur || !d_cond || !d_base ||
        !d_pred || !d_raw)
        return 3;

    /* 1. the linguistic encoder, word form */
    dsd_variance_encode_args ea;
    memset(&ea, 0, sizeof(ea));
    ea.struct_size = (int32_t)sizeof(ea);
    ea.B = B; ea.L = L; ea.W = W;
    ea.tokens = d_tokens; ea.word_div = d_word_div; ea.word_dur = d_word_dur; ea.languages = d_languages;
    ea.encoder_out = d_enc; ea.x_masks = d_masks;
    CHECK(NULL, dsd_variance_encode(v, &ea, NULL));
    if (print_sum("encoder_out", d_enc, (size_t)B * L * H)) return 3;

    /* 2. phoneme durations */
    dsd_variance_dur_args da;
    memset(&da, 0, sizeof(da));
    da.struct_size = (int32_t)sizeof(da);
    da.B = B; da.L = L;
    da.encoder_out = d_enc; da.x_masks = d_masks; da.ph_midi = d_ph_midi; da.spk_embed = d_spk; da.spk_rows = d_spk ? 1 : 0;
    da.ph_dur_pred = d_dur;
    CHECK(NULL, dsd_variance_dur(v, &da, NULL));
    if (print_sum("ph_dur_pred", d_dur, (size_t)B * L)) return 3;

    /* 3. the pitch condition (the editor's own ph_dur: aligning the prediction to the words is its business) */
    dsd_variance_pitch_cond_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.struct_size = (int32_t)sizeof(pa);
    pa.B = B; pa.L = L; pa.N = N; pa.T = T;
    pa.encoder_out = d_enc; pa.ph_dur = d_ph_dur; pa.note_midi = d_note_midi; pa.note_rest = d_note_rest; pa.note_dur = d_note_dur;
    pa.note_glide = c.use_glide_embed ? d_note_glide : NULL;
    pa.pitch = d_pitch; pa.retake = d_retake; pa.spk_embed = d_spk; pa.spk_rows = d_spk ? 1 : 0;
    pa.pitch_cond = d_cond; pa.base_pitch = d_base;
    CHECK(NULL, dsd_variance_pitch_cond(v, &pa, NULL));
    if (print_sum("pitch_cond", d_cond, (size_t)B * T * H) || print_sum("base_pitch", d_base, (size_t)B * T)) return 3;

    /* 4. the sampler stage: a reflow program from the library's own builder, on the borrowed handle */
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

    /* 5. the pitch itself */
    CHECK(NULL, dsd_variance_pitch_post(v, d_raw, d_base, B, T, d_pred, NULL));
    if (print_sum("pitch_pred", d_pred, (size_t)B * T)) return 3;

    if (n_var > 0) {
        /* 6. the variance condition on the predicted pitch, every variance retaken (its input curve does not count) */
        float* d_zero = (float*)to_device(NULL, sizeof(float) * (size_t)B * T);
        float* d_vcond = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * H);
        float* d_vraw = (float*)to_device(NULL, sizeof(float) * (size_t)B * n_var * T * (size_t)c.var_repeat_bins);
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
            d_curves[i] = (float*)to_device(NULL, sizeof(float) * (size_t)B * T);
            if (!d_curves[i]) return 3;
        }
        CHECK(NULL, dsd_variance_cond(v, &ca, NULL));
        if (print_sum("variance_cond", d_vcond, (size_t)B * T * H)) return 3;
        /* 7. its sampler stage, 8. the curves */
        dsd_handle* var_net = NULL;
        CHECK(NULL, dsd_variance_backbone(v, DSD_VAR_VARIANCES, &var_net));
        if (sample(var_net, prog, DOMAIN_VARIANCE_X_T, d_vcond, H, n_var, c.var_repeat_bins, lo, hi, d_vraw)) return 1;
        CHECK(NULL, dsd_variance_post(v, d_vraw, B, T, d_curves, NULL));
        for (int i = 0; i < n_var; ++i)
            if (print_sum(names[slot[i]], d_curves[i], (size_t)B * T)) return 3;
    }
    dsd_program_free(prog);
    dsd_variance_close(v);      /* releases the borrowed handles too */
    free(spk);
    return 0;
}
