/*
 * The acoustic model's staged twin from ONE model file in plain C: no Python, no torch, and no constant of the model in
 * this source - only include/dsdenoise.h and the HIP runtime for device memory.  Opens the file
 * (examples/pack_model.py --twin packs one), opens the acoustic object under a prefix (dsd_acoustic_open), reads every
 * size from dsd_acoustic_info, and runs a small synthetic segment through the stages an editor drives:
 *
 *   dsd_acoustic_condition (phonemes, durations, f0 -> condition, and the aux mel with shallow diffusion)
 *   -> dsd_acoustic_plan (depth and steps -> the start state and the loop)
 *   -> x from dsd_acoustic_start and dsd_noise_fill (the seeded x_T, mixed into the normalised aux mel in place)
 *   -> dsd_acoustic_sample -> mel
 *   -> dsd_vocode, when the file has a section "vocoder" of as many mel bins whose source needs no draws (mini_nsf)
 *
 * and prints the sum of every stage's output (`sum <name> <value>`).  tests/test_gpu_cacoustic.py compiles this with gcc,
 * runs it on the MI355X and compares the sums with the same chain driven from Python on the same file, inputs and seed.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_acoustic.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o acoustic_demo
 *   ./acoustic_demo model.dsdm ac
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

/* the segment: sizes, depth, steps and seed are the caller's, not the model's */
enum { B = 1, L = 6, T = 96, STEPS = 4 };
static const float DEPTH = 0.375f;
static const uint64_t SEED = 2026;
enum { DOMAIN_X_T = 1, DOMAIN_STEP = 2 };          /* the Python side's domains (dsd_noise_fill) */

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

static int draw(uint32_t domain, int n, int rows, int cols, const float* src, float src_scale, float scale, float* out) {
    dsd_noise_spec ns;
    memset(&ns, 0, sizeof(ns));
    ns.struct_size = (int32_t)sizeof(ns);
    ns.kind = DSD_NOISE_NORMAL;
    ns.domain = domain;
    ns.n = n; ns.B = B; ns.rows = rows; ns.cols = cols;
    ns.seeds = &SEED;
    ns.scale = scale;
    ns.src = src;
    ns.src_scale = src_scale;
    CHECK(NULL, dsd_noise_fill(0, &ns, out, NULL));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s model.dsdm prefix\n", argv[0]);
        return 2;
    }
    dsd_model_file* mf = NULL;
    CHECK(NULL, dsd_model_open(argv[1], &mf));
    dsd_acoustic* a = NULL;
    CHECK(NULL, dsd_acoustic_open(mf, argv[2], /*device=*/0, &a));
    dsd_acoustic_config c;
    CHECK(NULL, dsd_acoustic_info(a, &c));
    const int H = c.hidden_size, M = c.out_dims;
    printf("api v%d  hidden %d  vocab %d  mel bins %d  embed flags 0x%x  shallow %d  diffusion %d\n", dsd_api_version(), H, (int)c.vocab_size,
           M, (unsigned)c.embed_flags, (int)c.use_shallow_diffusion, (int)c.diffusion_type);

    /* the inputs an editor would have: phonemes, their durations, the pitch and the parameter curves */
    int64_t tokens[L], languages[L];
    for (int i = 0; i < L; ++i) {
        tokens[i] = 1 + (3 * i) % (c.vocab_size - 1);
        languages[i] = c.num_lang > 0 ? 1 + i % c.num_lang : 0;
    }
    tokens[L - 1] = 0;                                  /* a padding token: its duration does not count */
    const int64_t durations[L] = {20, 16, 0, 36, 24, 7};
    float f0[T], curve[T], gender[T], velocity[T];
    for (int t = 0; t < T; ++t) {
        f0[t] = (t >= 10 && t < 14) ? 0.0f : 180.0f + 0.5f * (float)t;
        curve[t] = -30.0f + 0.125f * (float)(t % 16);
        gender[t] = 0.3125f * (float)(t % 9 - 4);       /* -1.25 .. 1.25: clipped on both sides */
        velocity[t] = 0.25f + 0.125f * (float)(t % 20); /* 0.25 .. 2.625: likewise */
    }
    float* spk = (float*)malloc(sizeof(float) * (size_t)H);
    if (!spk) return 3;
    for (int h = 0; h < H; ++h) spk[h] = 0.015625f * (float)(h % 7 - 3);

    int64_t* d_tokens = (int64_t*)to_device(tokens, sizeof(tokens));
    int64_t* d_languages = (int64_t*)to_device(languages, sizeof(languages));
    int64_t* d_durations = (int64_t*)to_device(durations, sizeof(durations));
    float* d_f0 = (float*)to_device(f0, sizeof(f0));
    float* d_curve = (float*)to_device(curve, sizeof(curve));
    float* d_gender = (float*)to_device(gender, sizeof(gender));
    float* d_velocity = (float*)to_device(velocity, sizeof(velocity));
    float* d_spk = (float*)to_device(spk, sizeof(float) * (size_t)H);
    const size_t n_mel = (size_t)B * T * (size_t)M;
    float* d_cond = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * (size_t)H);
    float* d_aux = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_x = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_noise = (float*)to_device(NULL, sizeof(float) * n_mel);
    float* d_mel = (float*)to_device(NULL, sizeof(float) * n_mel);
    if (!d_tokens || !d_languages || !d_durations || !d_f0 || !d_curve || !d_gender || !d_velocity || !d_spk || !d_cond || !d_aux || !d_x ||
        !d_noise || !d_mel)
        return 3;

    /* 1. the condition (and the aux mel) */
    dsd_acoustic_condition_args ca;
    memset(&ca, 0, sizeof(ca));
    ca.struct_size = (int32_t)sizeof(ca);
    ca.B = B; ca.L = L; ca.T = T;
    ca.tokens = d_tokens; ca.durations = d_durations; ca.f0 = d_f0;
    for (int i = 0; i < 4; ++i)
        if ((c.embed_flags >> i) & 1u) ca.curves[i] = d_curve;
    if (c.embed_flags & DSD_EMBED_KEY_SHIFT) ca.gender = d_gender;
    if (c.embed_flags & DSD_EMBED_SPEED) ca.velocity = d_velocity;
    if (c.use_spk_id) { ca.spk_embed = d_spk; ca.spk_rows = 1; }
    if (c.use_lang_id) ca.languages = d_languages;
    ca.condition = d_cond;
    ca.aux_mel = c.use_shallow_diffusion ? d_aux : NULL;
    CHECK(NULL, dsd_acoustic_condition(a, &ca, NULL));
    if (print_sum("condition", d_cond, (size_t)B * T * (size_t)H)) return 3;
    if (c.use_shallow_diffusion && print_sum("aux_mel", d_aux, n_mel)) return 3;

    /* 2. the plan: from the aux mel at DEPTH with shallow diffusion, from noise without */
    dsd_acoustic_plan_t plan;
    CHECK(NULL, dsd_acoustic_plan(&c, c.use_shallow_diffusion ? DEPTH : -1.0f, STEPS, &plan));
    printf("plan: start %d  t_max %d  speedup %d  t_start %.9g  step noise %d\n", (int)plan.start, (int)plan.t_max, (int)plan.speedup,
           (double)plan.t_start, (int)plan.n_step_noise);

    /* 3. the start state, x_T under the seed */
    if (plan.start == DSD_AC_START_NOISE) {
        if (draw(DOMAIN_X_T, 1, M, T, NULL, 0.0f, 1.0f, d_noise)) return 1;
        CHECK(NULL, dsd_acoustic_start(a, &plan, NULL, d_noise, B, T, d_x, NULL));
    } else {
        CHECK(NULL, dsd_acoustic_start(a, &plan, d_aux, NULL, B, T, d_x, NULL));       /* the normalised, transposed aux mel */
        if (plan.start == DSD_AC_START_MIX && draw(DOMAIN_X_T, 1, M, T, d_x, plan.src_scale, plan.noise_scale, d_x)) return 1;
    }
    if (print_sum("x", d_x, n_mel)) return 3;
    float* d_step = NULL;
    if (plan.n_step_noise > 0) {                        /* the ancestral sampler: one tensor per step, streams 0 .. */
        d_step = (float*)to_device(NULL, sizeof(float) * n_mel * (size_t)plan.n_step_noise);
        if (!d_step || draw(DOMAIN_STEP, plan.n_step_noise, M, T, NULL, 0.0f, 1.0f, d_step)) return 1;
    }

    /* 4. the sampler stage */
    CHECK(NULL, dsd_acoustic_sample(a, &plan, d_cond, d_x, d_step, B, T, 0, d_mel, NULL));
    if (print_sum("mel", d_mel, n_mel)) return 3;

    /* 5. the waveform, when the file brings a vocoder for these mels that needs no draws */
    const int voc_i = dsd_model_find(mf, "vocoder");
    if (voc_i >= 0) {
        dsd_model_section_info si;
        dsd_vocoder_config vc;
        CHECK(NULL, dsd_model_section(mf, voc_i, &si));
        if (si.kind == DSD_VOC_NSF_HIFIGAN) {
            CHECK(NULL, dsd_model_config(mf, voc_i, &vc, (int32_t)sizeof(vc)));
            if (vc.num_mels == M && vc.mini_nsf && vc.noise_sigma == 0.0f) {
                int64_t upp = 1;
                for (int32_t i = 0; i < vc.n_ups; ++i) upp *= vc.upsample_rates[i];
                dsd_handle* voc = NULL;
                CHECK(NULL, dsd_model_create(mf, voc_i, 0, &voc));
                float* d_wav = (float*)to_device(NULL, sizeof(float) * (size_t)B * T * (size_t)upp);
                if (!d_wav) return 3;
                /* mel is [B, T, M] natural-log (the sampler stage has applied the mel base); the vocoder reads it by strides */
                CHECK(voc, dsd_vocode(voc, d_mel, B, T, (int64_t)T * M, 1, M, d_f0, NULL, NULL, NULL, d_wav, NULL));
                if (print_sum("wav", d_wav, (size_t)B * T * (size_t)upp)) return 3;
                dsd_destroy(voc);
            } else {
                printf("vocoder: %d mel bins, mini_nsf %d, noise_sigma %g - not vocoded here\n", (int)vc.num_mels, (int)vc.mini_nsf,
                       (double)vc.noise_sigma);
            }
        }
    }
    dsd_model_close(mf);
    dsd_acoustic_close(a);      /* releases the borrowed handles and the cached programs too */
    free(spk);
    return 0;
}
