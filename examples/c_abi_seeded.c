/*
 * A seeded run from plain C: the random draws come from the library (dsd_noise_fill), not from a generator the caller
 * has to write, run on the host and upload.  The same small WaveNet denoiser as c_abi_denoise.c; x_T is drawn on the
 * device from one 64-bit seed per batch item, and a 6-step program of the ancestral-DDPM shape
 *     x <- a_k * x + b_k * model(x, t_k) + c_k * noise_k
 * takes its six noise tensors from ONE dsd_noise_fill call (n = 6: streams 0..5 of the step domain).  The draws are a
 * pure function of (seed, domain, stream, row, column) - include/dsdenoise.h has the specification - so any caller that
 * passes the same seeds gets the same bits.  tests/test_gpu_noise.py compiles this with gcc, runs it on the MI355X and
 * compares the printed x_T values with the numpy restatement of the generator.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_seeded.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o seeded
 *   ./seeded weights.bin inputs.bin outputs.bin
 *
 * weights.bin: int32 n, then n records { int32 name_len, name bytes, int32 ndim, int64 shape[ndim], float data[] }
 * inputs.bin : int32 B, T, H, M; uint64 seed[B]; float cond[B*H*T]
 * outputs.bin: float x_T[B*M*T], sample[B*M*T]
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsdenoise.h"

#define CHECK(call)                                                                     \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != 0) {                                                                 \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dsd_last_error(h));     \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

#define DOMAIN_X_T 1u   /* the tags the Python side uses (diffsinger_amd/noise.py): any caller-chosen values keep */
#define DOMAIN_STEP 2u  /* the tensors drawn under one seed apart                                                 */
#define N_STEPS 6

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s weights.bin inputs.bin outputs.bin\n", argv[0]);
        return 2;
    }
    dsd_handle* h = NULL;
    dsd_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = (int32_t)sizeof(cfg);
    cfg.backbone = DSD_BACKBONE_WAVENET;
    cfg.n_feats = 1;
    cfg.num_layers = 4;
    cfg.num_channels = 64;
    cfg.dilation_cycle_length = 2;
    cfg.device = 0;

    FILE* fi = fopen(argv[2], "rb");
    if (!fi) return 2;
    int32_t dims[4];
    if (fread(dims, sizeof(int32_t), 4, fi) != 4) return 2;
    const int B = dims[0], T = dims[1], H = dims[2], M = dims[3];
    if (B < 1 || B > 64) return 2;
    cfg.in_dims = M;
    cfg.hidden_size = H;
    const size_t n_cond = (size_t)B * H * T, n_x = (size_t)B * M * T;
    uint64_t seeds[64];
    float* cond = (float*)malloc(n_cond * sizeof(float));
    if (fread(seeds, sizeof(uint64_t), (size_t)B, fi) != (size_t)B || fread(cond, sizeof(float), n_cond, fi) != n_cond) return 2;
    fclose(fi);

    CHECK(dsd_create(&cfg, &h));
    FILE* fw = fopen(argv[1], "rb");
    if (!fw) return 2;
    int32_t n_tensors = 0;
    if (fread(&n_tensors, sizeof(int32_t), 1, fw) != 1) return 2;
    for (int32_t i = 0; i < n_tensors; ++i) {
        int32_t name_len, ndim;
        char name[256];
        int64_t shape[4];
        if (fread(&name_len, sizeof(int32_t), 1, fw) != 1 || name_len <= 0 || name_len > 255) return 2;
        if (fread(name, 1, (size_t)name_len, fw) != (size_t)name_len) return 2;
        name[name_len] = 0;
        if (fread(&ndim, sizeof(int32_t), 1, fw) != 1 || ndim < 1 || ndim > 4) return 2;
        if (fread(shape, sizeof(int64_t), (size_t)ndim, fw) != (size_t)ndim) return 2;
        size_t numel = 1;
        for (int d = 0; d < ndim; ++d) numel *= (size_t)shape[d];
        float* data = (float*)malloc(numel * sizeof(float));
        if (fread(data, sizeof(float), numel, fw) != numel) return 2;
        CHECK(dsd_load_weight(h, name, data, shape, ndim, /*on_device=*/0));
        free(data);
    }
    fclose(fw);
    CHECK(dsd_finalize_weights(h));

    float *d_cond = NULL, *d_xT = NULL, *d_noise = NULL, *d_samp = NULL;
    if (hipMalloc((void**)&d_cond, n_cond * sizeof(float)) != hipSuccess ||
        hipMemcpy(d_cond, cond, n_cond * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void**)&d_xT, n_x * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_noise, N_STEPS * n_x * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_samp, n_x * sizeof(float)) != hipSuccess)
        return 3;

    /* x_T [B, 1, M, T]: one draw (n = 1) of B items, M rows of T columns each, item b under seeds[b] */
    dsd_noise_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.struct_size = (int32_t)sizeof(spec);
    spec.kind = DSD_NOISE_NORMAL;
    spec.domain = DOMAIN_X_T;
    spec.first_stream = 0;
    spec.n = 1;
    spec.B = B;
    spec.rows = M;
    spec.cols = T;
    spec.seeds = seeds;
    spec.scale = 1.0f;
    spec.src = NULL;
    spec.src_scale = 0.0f;
    CHECK(dsd_noise_fill(cfg.device, &spec, d_xT, NULL));
    /* the six step-noise tensors [6, B, 1, M, T] in one call: tensor k is stream k of the step domain */
    spec.domain = DOMAIN_STEP;
    spec.n = N_STEPS;
    CHECK(dsd_noise_fill(cfg.device, &spec, d_noise, NULL));

    CHECK(dsd_prepare_cond(h, d_cond, B, T, (int64_t)H * T, T, 1, NULL));
    dsd_eval evals[N_STEPS];
    memset(evals, 0, sizeof(evals));
    for (int k = 0; k < N_STEPS; ++k) {
        evals[k].x_buf = 0;
        evals[k].t = 50.0f - 10.0f * (float)k;
        evals[k].n_out = 1;
        evals[k].out[0].dst = 0;
        evals[k].out[0].n_terms = k + 1 < N_STEPS ? 3 : 2;         /* the last step adds no noise, as in p_sample at t = 0 */
        evals[k].out[0].terms[0].src = 0;
        evals[k].out[0].terms[0].coef = 0.95f + 0.005f * (float)k;
        evals[k].out[0].terms[1].src = DSD_SRC_MODEL;
        evals[k].out[0].terms[1].coef = -0.15f + 0.02f * (float)k;
        evals[k].out[0].terms[2].src = DSD_SRC_NOISE_BASE - k;
        evals[k].out[0].terms[2].coef = 0.1f - 0.015f * (float)k;
    }
    dsd_program prog;
    prog.n_bufs = 1;
    prog.result_buf = 0;
    prog.n_evals = N_STEPS;
    prog.n_noise = N_STEPS;
    prog.evals = evals;
    CHECK(dsd_sample(h, &prog, d_xT, d_noise, d_samp, NULL, NULL, DSD_SAMPLE_GRAPH, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 3;

    float* xT = (float*)malloc(n_x * sizeof(float));
    float* samp = (float*)malloc(n_x * sizeof(float));
    if (hipMemcpy(xT, d_xT, n_x * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(samp, d_samp, n_x * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return 3;
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    fwrite(xT, sizeof(float), n_x, fo);
    fwrite(samp, sizeof(float), n_x, fo);
    fclose(fo);

    double sum = 0.0, sum_abs = 0.0;
    for (size_t i = 0; i < n_x; ++i) {
        sum += samp[i];
        sum_abs += samp[i] < 0 ? -samp[i] : samp[i];
    }
    printf("x_T %.9g %.9g %.9g %.9g\n", xT[0], xT[1], xT[2], xT[3]);
    printf("sample checksum %.9g  mean |x| %.9g\n", sum, sum_abs / (double)n_x);
    dsd_destroy(h);
    return 0;
}
