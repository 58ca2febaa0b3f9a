/*
 * A whole sampler from plain C: the library builds the program.  The same small WaveNet denoiser as c_abi_denoise.c and
 * c_abi_seeded.c, but nothing about the sampler is written out by hand here:
 *   1. dsd_ddpm_tables_fill   the twelve schedule buffers of GaussianDiffusion (linear, 1000 steps, max_beta 0.01)
 *   2. dsd_program_build      DPM-Solver++ 2M from t_max = 1000 with speed-up 50: 20 evaluations
 *   3. dsd_noise_fill         x_T, one 64-bit seed per batch item
 *   4. dsd_sample             the loop, replayed from a hipGraph
 *   5. dsd_program_free
 *   6. the sample to outputs.bin
 * No Python in the process and no solver arithmetic in the caller.  tests/test_gpu_cprogram.py compiles this with gcc, runs
 * it on the MI355X and compares the sample with the same sampler run from Python on the same seeds.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_sampler.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o sampler
 *   ./sampler weights.bin inputs.bin outputs.bin
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

#define DOMAIN_X_T 1u   /* the tag the Python side uses for x_T (diffsinger_amd/noise.py) */
#define TIMESTEPS 1000
#define SPEEDUP 50      /* 1000 -> 20 steps */

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

    float *d_cond = NULL, *d_xT = NULL, *d_samp = NULL;
    if (hipMalloc((void**)&d_cond, n_cond * sizeof(float)) != hipSuccess ||
        hipMemcpy(d_cond, cond, n_cond * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void**)&d_xT, n_x * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_samp, n_x * sizeof(float)) != hipSuccess)
        return 3;

    /* 1. the schedule: [12][TIMESTEPS] host floats (a checkpoint's own buffers, in the same order, would do as well) */
    float* tables = (float*)malloc((size_t)DSD_DDPM_TABLES * TIMESTEPS * sizeof(float));
    if (!tables) return 3;
    if (dsd_ddpm_tables_fill(DSD_SCHEDULE_LINEAR, TIMESTEPS, 0.01, tables) != DSD_OK) {
        fprintf(stderr, "dsd_ddpm_tables_fill: %s\n", dsd_last_error(NULL));
        return 1;
    }

    /* 2. the program: built once, good for any number of dsd_sample calls at any batch shape */
    dsd_sampler_spec sampler;
    memset(&sampler, 0, sizeof(sampler));
    sampler.struct_size = (int32_t)sizeof(sampler);
    sampler.sampler = DSD_SAMPLER_DPM_SOLVER_PP;
    sampler.timesteps = TIMESTEPS;
    sampler.tables = tables;
    sampler.t_max = TIMESTEPS;
    sampler.speedup = SPEEDUP;
    dsd_program* prog = NULL;
    if (dsd_program_build(&sampler, &prog) != DSD_OK) {
        fprintf(stderr, "dsd_program_build: %s\n", dsd_last_error(NULL));      /* handle-free: the message is under NULL */
        return 1;
    }
    free(tables);                                                              /* the program does not point into them */

    /* 3. x_T [B, 1, M, T]: one draw (n = 1) of B items, M rows of T columns each, item b under seeds[b] */
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
    if (dsd_noise_fill(cfg.device, &spec, d_xT, NULL) != DSD_OK) {
        fprintf(stderr, "dsd_noise_fill: %s\n", dsd_last_error(NULL));
        return 1;
    }

    /* 4. the loop */
    CHECK(dsd_prepare_cond(h, d_cond, B, T, (int64_t)H * T, T, 1, NULL));
    CHECK(dsd_sample(h, prog, d_xT, NULL, d_samp, NULL, NULL, DSD_SAMPLE_GRAPH, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    const int n_evals = prog->n_evals, n_bufs = prog->n_bufs;
    /* 5. */
    dsd_program_free(prog);

    /* 6. */
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
    printf("program %d evaluations, %d buffers\n", n_evals, n_bufs);
    printf("sample checksum %.9g  mean |x| %.9g\n", sum, sum_abs / (double)n_x);
    dsd_destroy(h);
    return 0;
}
