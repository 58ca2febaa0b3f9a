/*
 * A multi-speaker project rendered from ONE model file in plain C: three segments of different lengths, each with its own
 * seed, in ONE padded batch from phonemes to int16 samples - no Python, no torch, no solver arithmetic, no constant of the
 * model and no draw made on the host in this source; only include/dsdenoise.h and the HIP runtime for device memory.
 * The file (examples/pack_model.py --twin packs one) holds a multi-speaker acoustic model under a prefix and a section
 * "vocoder": an NSF-HiFiGAN for as many mel bins with a SineGen source (and, if it likes, noise_sigma > 0).
 *
 *   1. dsd_acoustic_set_lengths      the segments' frame counts: every item comes out as it would alone
 *   2. dsd_acoustic_spk_mix          the speaker mixes from the table inside the file: a static two-speaker mix for
 *                                    segment 0, a per-frame cross-fade for segment 1, one speaker (and a padding speaker
 *                                    with value 0) for segment 2
 *   3. dsd_acoustic_condition
 *   4. dsd_acoustic_plan
 *   5. dsd_acoustic_start + dsd_noise_fill (DSD_DOMAIN_X_T, one seed per segment, mixed in place)
 *   6. dsd_acoustic_sample
 *   7. dsd_vocode_seeded             with the lengths and the same seeds: the vocoder's draws are made inside its kernels
 *   8. dsd_track_plan / _place / _peak / _export to int16
 *
 * and prints `sum <name> <value>` over the valid frames of every stage's output, the track's total, peak and the sum of
 * |sample| of the int16 track.  tests/test_gpu_cproject.py compiles this with gcc, runs it on the MI355X and compares the
 * figures with the same chain driven from Python on the same file, inputs and seeds.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_project.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o project_demo
 *   ./project_demo model.dsdm ac project.s16
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

/* the project: sizes, depth, steps and seeds are the caller's, not the model's */
enum { B = 3, L = 6, T = 48, STEPS = 4, N_SPK = 2 };
static const int32_t LENGTHS[B] = {48, 17, 30};          /* frames per segment; the batch is padded to T */
static const uint64_t SEEDS[B] = {2026, 7, 0x123456789abcdefull};
static const float DEPTH = 0.375f;

static void* to_device(const void* src, size_t bytes) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    if (src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
    if (!src && hipMemset(d, 0, bytes) != hipSuccess) return NULL;
    return d;
}

/* the sum over every item's valid rows of a [B, T, cols] tensor: what lies past an item's end is unspecified */
static int print_sum(const char* name, const float* dev, size_t cols) {
    const size_t n = (size_t)B * T * cols;
    float* host = (float*)malloc(n * sizeof(float));
    if (!host || hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double sum = 0.0;
    for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)LENGTHS[b] * cols; ++i) sum += (double)host[(size_t)b * T * cols + i];
    printf("sum %s %.17g\n", name, sum);
    free(host);
    return 0;
}

static int draw(uint32_t domain, int n, int rows, int cols, const float* src, float src_scale, float scale, float* out) {
    dsd_noise_spec ns;
    memset(&ns, 0, sizeof(ns));
    ns.struct_size = (int32_t)sizeof(ns);
    ns.kind = DSD_NOISE_NORMAL;
    ns.domain = domain;
    ns.n = n; ns.B = B; ns.rows = rows; ns.cols = cols;
    ns.seeds = SEEDS;                                   /* one per segment: a segment draws what it draws alone */
    ns.scale = scale;
    ns.src = src;
    ns.src_scale = src_scale;
    CHECK(NULL, dsd_noise_fill(0, &ns, out, NULL));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s model.dsdm prefix out.s16\n", argv[0]);
        return 2;
    }
    dsd_model_file* mf = NULL;
    CHECK(NULL, dsd_model_open(argv[1], &mf));
    dsd_acoustic* a = NULL;
    CHECK(NULL, dsd_acoustic_open(mf, argv[2], /*device=*/0, &a));
    dsd_acoustic_config c;
    CHECK(NULL, dsd_acoustic_info(a, &c));
    const int H = c.hidden_size, M = c.out_dims;
    printf("api v%d  hidden %d  mel bins %d  speakers %d  embed flags 0x%x  shallow %d  diffusion %d\n", dsd_api_version(), H, M,
           (int)c.num_spk, (unsigned)c.embed_flags, (int)c.use_shallow_diffusion, (int)c.diffusion_type);
    const int voc_i = dsd_model_find(mf, "vocoder");
    if (voc_i < 0 || !c.use_spk_id || c.num_spk < 1) {
        fprintf(stderr, "the file needs a multi-speaker acoustic model and a section \"vocoder\"\n");
        return 2;
    }
    dsd_vocoder_config vc;
    CHECK(NULL, dsd_model_config(mf, voc_i, &vc, (int32_t)sizeof(vc)));
    if (vc.num_mels != M) {
        fprintf(stderr, "the vocoder takes %d mel bins, the acoustic model gives %d\n", (int)vc.num_mels, M);
        return 2;
    }
    int64_t upp = 1;
    for (int32_t i = 0; i < vc.n_ups; ++i) upp *= vc.upsample_rates[i];
    dsd_handle* voc = NULL;
    CHECK(NULL, dsd_model_create(mf, voc_i, 0, &voc));

    /* the inputs an editor would have, per segment: phonemes, their durations, the pitch and the parameter curves.  Every
       segment's durations total its length; what lies past its end in the padded buffers is junk, not zeros */
    static const int64_t durations[B][L] = {{10, 8, 6, 12, 7, 5}, {5, 4, 9, 8, 0, 0}, {6, 6, 6, 6, 6, 0}};
    int64_t tokens[B][L], languages[B][L];
    float f0[B][T], curve[B][T], gender[B][T], velocity[B][T], mix[B][T][N_SPK];
    int32_t ids[B][N_SPK];
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < L; ++i) {
            tokens[b][i] = 1 + (3 * i + b) % (c.vocab_size - 1);
            languages[b][i] = c.num_lang > 0 ? 1 + (i + b) % c.num_lang : 0;
        }
        for (int t = 0; t < T; ++t) {
            const int in = t < LENGTHS[b];
            f0[b][t] = !in ? 3000.0f : ((t >= 10 && t < 14) ? 0.0f : 160.0f + 20.0f * (float)b + 0.5f * (float)t);
            curve[b][t] = in ? -30.0f + 0.125f * (float)((t + b) % 16) : 99.0f;
            gender[b][t] = in ? 0.3125f * (float)((t + b) % 9 - 4) : -7.0f;
            velocity[b][t] = in ? 0.25f + 0.125f * (float)((t + b) % 20) : 50.0f;
        }
    }
    tokens[1][2] = 0;                                   /* a padding token with a duration: it does not count */
    tokens[1][4] = tokens[1][5] = 0;
    tokens[2][5] = 0;
    /* the speaker mixes, proportions per frame (normalised by the library): segment 0 a static 1 : 3 mix of the first and the
       last speaker, segment 1 a cross-fade from the last to the first, segment 2 the last speaker and a padding speaker */
    ids[0][0] = 0; ids[0][1] = c.num_spk - 1;
    ids[1][0] = c.num_spk - 1; ids[1][1] = 0;
    ids[2][0] = c.num_spk - 1; ids[2][1] = 0;
    for (int t = 0; t < T; ++t) {
        mix[0][t][0] = 1.0f; mix[0][t][1] = 3.0f;
        mix[1][t][0] = (float)(T - t); mix[1][t][1] = (float)t;
        mix[2][t][0] = 2.0f; mix[2][t][1] = 0.0f;
    }

    int64_t* d_tokens = (int64_t*)to_device(tokens, sizeof(tokens));
    int64_t* d_languages = (int64_t*)to_device(languages, sizeof(languages));
    int64_t* d_durations = (int64_t*)to_device(durations, sizeof(durations));
    float* d_f0 = (float*)to_device(f0, sizeof(f0));
    float* d_curve = (float*)to_device(curve, sizeof(curve));
    float* d_gender = (float*)to_device(gender, sizeof(gender));
    float* d_velocity = (float*)to_device(velocity, sizeof(velocity));
    float* d_mix = (float*)to_device(mix, sizeof(mix));
    const size_t n_mel = (size_t)B * T * (size_t)M, n_wav = (size_t)B * T * (size_t)upp;
    float* d_spk = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * (size_t)H);
    float* d_cond = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * (size_t)H);
    float* d_aux = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_x = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_noise = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_mel = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_wav = (float*)to_device(NULL, sizeof(float) * n_wav);
    if (!d_tokens || !d_languages || !d_durations || !d_f0 || !d_curve || !d_gender || !d_velocity || !d_mix || !d_spk || !d_cond ||
        !d_aux || !d_x || !d_noise || !d_mel || !d_wav)
        return 3;

    /* 1. the lengths, for every stage call that follows */
    CHECK(NULL, dsd_acoustic_set_lengths(a, LENGTHS, B, NULL));

    /* 2. the speaker mixes */
    dsd_spk_mix_args sm;
    memset(&sm, 0, sizeof(sm));
    sm.struct_size = (int32_t)sizeof(sm);
    sm.B = B; sm.rows = T; sm.N = N_SPK;
    sm.ids = &ids[0][0];
    sm.values = d_mix;
    sm.normalize = 1;
    sm.out = d_spk;
    CHECK(NULL, dsd_acoustic_spk_mix(a, &sm, NULL));
    if (print_sum("spk_mix", d_spk, (size_t)H)) return 3;

    /* 3. the condition (and the aux mel) */
    dsd_acoustic_condition_args ca;
    memset(&ca, 0, sizeof(ca));
    ca.struct_size = (int32_t)sizeof(ca);
    ca.B = B; ca.L = L; ca.T = T;
    ca.tokens = d_tokens; ca.durations = d_durations; ca.f0 = d_f0;
    for (int i = 0; i < 4; ++i)
        if ((c.embed_flags >> i) & 1u) ca.curves[i] = d_curve;
    if (c.embed_flags & DSD_EMBED_KEY_SHIFT) ca.gender = d_gender;
    if (c.embed_flags & DSD_EMBED_SPEED) ca.velocity = d_velocity;
    ca.spk_embed = d_spk; ca.spk_rows = T;
    if (c.use_lang_id) ca.languages = d_languages;
    ca.condition = d_cond;
    ca.aux_mel = c.use_shallow_diffusion ? d_aux : NULL;
    CHECK(NULL, dsd_acoustic_condition(a, &ca, NULL));
    if (print_sum("condition", d_cond, (size_t)H)) return 3;
    if (c.use_shallow_diffusion && print_sum("aux_mel", d_aux, (size_t)M)) return 3;

    /* 4. the plan: from the aux mel at DEPTH with shallow diffusion, from noise without */
    dsd_acoustic_plan_t plan;
    CHECK(NULL, dsd_acoustic_plan(&c, c.use_shallow_diffusion ? DEPTH : -1.0f, STEPS, &plan));
    printf("plan: start %d  t_max %d  speedup %d  t_start %.9g  step noise %d\n", (int)plan.start, (int)plan.t_max, (int)plan.speedup,
           (double)plan.t_start, (int)plan.n_step_noise);

    /* 5. the start state, x_T under each segment's seed */
    if (plan.start == DSD_AC_START_NOISE) {
        if (draw(DSD_DOMAIN_X_T, 1, M, T, NULL, 0.0f, 1.0f, d_noise)) return 1;
        CHECK(NULL, dsd_acoustic_start(a, &plan, NULL, d_noise, B, T, d_x, NULL));
    } else {
        CHECK(NULL, dsd_acoustic_start(a, &plan, d_aux, NULL, B, T, d_x, NULL));       /* the normalised, transposed aux mel */
        if (plan.start == DSD_AC_START_MIX && draw(DSD_DOMAIN_X_T, 1, M, T, d_x, plan.src_scale, plan.noise_scale, d_x)) return 1;
    }
    float* d_step = NULL;
    if (plan.n_step_noise > 0) {                        /* the ancestral sampler: one tensor per step, streams 0 .. */
        d_step = (float*)to_device(NULL, sizeof(float) * n_mel * (size_t)plan.n_step_noise);
        if (!d_step || draw(DSD_DOMAIN_STEP, plan.n_step_noise, M, T, NULL, 0.0f, 1.0f, d_step)) return 1;
    }

    /* 6. the sampler stage */
    CHECK(NULL, dsd_acoustic_sample(a, &plan, d_cond, d_x, d_step, B, T, 0, d_mel, NULL));
    if (print_sum("mel", d_mel, (size_t)M)) return 3;

    /* 7. the waveforms: mel is [B, T, M] natural-log (the sampler stage has applied the mel base), read by strides; the
          vocoder's phases and noises are drawn inside its kernels from the segments' seeds */
    dsd_vocode_seeded_args va;
    memset(&va, 0, sizeof(va));
    va.struct_size = (int32_t)sizeof(va);
    va.B = B; va.T = T;
    va.vocoder = voc;
    va.mel = d_mel; va.stride_b = (int64_t)T * M; va.stride_m = 1; va.stride_t = M;
    va.lengths = LENGTHS;
    va.f0 = d_f0;
    va.seeds = SEEDS;
    va.wav_out = d_wav;
    CHECK(voc, dsd_vocode_seeded(&va, NULL));
    if (print_sum("wav", d_wav, (size_t)upp)) return 3;

    /* 8. the track: segment k starts 0.85 of segment k - 1's duration after it (segments 0 and 1 overlap and are cross-faded)
          or 1.2 of it (a gap before segment 2) */
    const double rate = (double)vc.sampling_rate;
    int64_t samples[B], starts[B], prev_ends[B], total = 0;
    double offsets[B];
    for (int b = 0; b < B; ++b) samples[b] = (int64_t)LENGTHS[b] * upp;
    offsets[0] = 0.0;
    offsets[1] = 0.85 * (double)samples[0] / rate;
    offsets[2] = offsets[1] + 1.2 * (double)samples[1] / rate;
    CHECK(NULL, dsd_track_plan(B, offsets, samples, vc.sampling_rate, starts, prev_ends, &total));
    double *d_track = NULL, *d_peak = NULL;
    int16_t* d_pcm = NULL;
    if (hipMalloc((void**)&d_track, (size_t)total * sizeof(double)) != hipSuccess || hipMalloc((void**)&d_peak, sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_pcm, (size_t)total * sizeof(int16_t)) != hipSuccess)
        return 3;
    for (int b = 0; b < B; ++b)
        CHECK(NULL, dsd_track_place(0, d_track, total, starts[b], prev_ends[b], d_wav + (size_t)b * T * (size_t)upp, samples[b], NULL));
    CHECK(NULL, dsd_track_peak(0, d_track, total, d_peak, NULL));
    CHECK(NULL, dsd_track_export(0, d_track, total, DSD_TRACK_PCM, d_peak, d_pcm, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    double peak = 0.0;
    int16_t* pcm = (int16_t*)malloc((size_t)total * sizeof(int16_t));
    if (!pcm || hipMemcpy(&peak, d_peak, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pcm, d_pcm, (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess)
        return 3;
    FILE* fo = fopen(argv[3], "wb");
    if (!fo || fwrite(pcm, sizeof(int16_t), (size_t)total, fo) != (size_t)total) return 2;
    fclose(fo);
    long long checksum = 0;
    for (int64_t i = 0; i < total; ++i) checksum += pcm[i] < 0 ? -(long long)pcm[i] : pcm[i];
    printf("total %lld\n", (long long)total);
    printf("peak %.17g\n", peak);
    printf("checksum %lld\n", checksum);

    free(pcm);
    dsd_destroy(voc);
    dsd_model_close(mf);
    dsd_acoustic_close(a);      /* releases the borrowed handles and the cached programs too */
    return 0;
}
