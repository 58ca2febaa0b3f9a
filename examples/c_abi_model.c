/*
 * From ONE model file to a waveform in plain C: no Python, no torch, no constant of the model in this source - only
 * include/dsdenoise.h and the HIP runtime for device memory.  Opens a model file (diffsinger_amd/modelfile.py or
 * examples/pack_model.py writes one), prints its sections and metadata, creates the handles of the sections "denoiser"
 * and "vocoder" with dsd_model_create, reads every size it needs from the stored configs (dsd_model_config), runs
 * dsd_prepare_cond and one backbone evaluation (dsd_denoise), vocodes that evaluation's output as a mel with the
 * file's vocoder (dsd_vocode; a mini_nsf generator: its source is deterministic, so no draws are needed) and writes both
 * outputs.  tests/test_gpu_modelfile.py compiles this with gcc, runs it on the MI355X and compares both outputs with the
 * Python wrappers on the same inputs.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_model.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/diffsinger_amd -o model_demo
 *   ./model_demo model.dsdm inputs.bin outputs.bin
 *
 * inputs.bin : int32 B, T; float cond[B*H*T] ([B, H, T]), x[B*M*T] ([B, 1, M, T]), t[B], f0[B*T] - H = the denoiser's
 *              hidden_size and M = its in_dims, both read from the file
 * outputs.bin: float denoised[B*M*T], wav[B * T * prod(upsample_rates)]
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

static void* to_device(const void* src, size_t bytes) {
    void* d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
    return d;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s model.dsdm inputs.bin outputs.bin\n", argv[0]);
        return 2;
    }
    /* 1. the file: sections and metadata */
    dsd_model_file* mf = NULL;
    CHECK(NULL, dsd_model_open(argv[1], &mf));
    int32_t n_sections = 0, n_meta = 0;
    CHECK(NULL, dsd_model_count(mf, &n_sections, &n_meta));
    printf("api v%d  %d sections  %d metadata entries\n", dsd_api_version(), (int)n_sections, (int)n_meta);
    for (int32_t i = 0; i < n_sections; ++i) {
        dsd_model_section_info si;
        CHECK(NULL, dsd_model_section(mf, i, &si));
        printf("section %d: \"%s\" kind %d, %d tensors, %lld floats\n", (int)i, si.name, (int)si.kind, (int)si.n_tensors,
               (long long)si.total_floats);
    }
    for (int32_t k = 0; k < n_meta; ++k) {
        const char *key, *value;
        CHECK(NULL, dsd_model_meta_at(mf, k, &key, &value));
        printf("meta \"%s\" = \"%s\"\n", key, value);
    }

    /* 2. the two handles, 3. every size from the stored configs */
    const int den_i = dsd_model_find(mf, "denoiser"), voc_i = dsd_model_find(mf, "vocoder");
    if (den_i < 0 || voc_i < 0) {
        fprintf(stderr, "%s\n", dsd_last_error(NULL));
        return 1;
    }
    dsd_config dc;
    dsd_vocoder_config vc;
    CHECK(NULL, dsd_model_config(mf, den_i, &dc, (int32_t)sizeof(dc)));       /* refuses a section of another kind: its size differs */
    CHECK(NULL, dsd_model_config(mf, voc_i, &vc, (int32_t)sizeof(vc)));
    const int M = dc.in_dims, H = dc.hidden_size;
    int64_t upp = 1;
    for (int32_t i = 0; i < vc.n_ups; ++i) upp *= vc.upsample_rates[i];
    printf("denoiser: in_dims %d hidden_size %d  vocoder: num_mels %d hop %lld\n", M, H, (int)vc.num_mels, (long long)upp);
    if (dc.n_feats != 1 || vc.num_mels != M || !vc.mini_nsf || vc.noise_sigma > 0.0f) {
        fprintf(stderr, "this example vocodes the denoiser's output without random draws: it needs n_feats 1, num_mels == in_dims, "
                        "a mini_nsf generator and noise_sigma 0\n");
        return 1;
    }
    dsd_handle *den = NULL, *voc = NULL;
    CHECK(NULL, dsd_model_create(mf, den_i, /*device=*/0, &den));
    CHECK(NULL, dsd_model_create(mf, voc_i, /*device=*/0, &voc));
    dsd_model_close(mf);        /* the handles hold their own copies of the weights */

    FILE* fi = fopen(argv[2], "rb");
    if (!fi) return 2;
    int32_t dims[2];
    if (fread(dims, sizeof(int32_t), 2, fi) != 2 || dims[0] < 1 || dims[1] < 1) return 2;
    const int B = dims[0], T = dims[1];
    const size_t n_cond = (size_t)B * H * T, n_x = (size_t)B * M * T, n_f0 = (size_t)B * T, n_wav = (size_t)B * T * (size_t)upp;
    float* cond = (float*)malloc(n_cond * sizeof(float));
    float* x = (float*)malloc(n_x * sizeof(float));
    float* t = (float*)malloc((size_t)B * sizeof(float));
    float* f0 = (float*)malloc(n_f0 * sizeof(float));
    if (!cond || !x || !t || !f0) return 3;
    if (fread(cond, sizeof(float), n_cond, fi) != n_cond || fread(x, sizeof(float), n_x, fi) != n_x ||
        fread(t, sizeof(float), (size_t)B, fi) != (size_t)B || fread(f0, sizeof(float), n_f0, fi) != n_f0)
        return 2;
    fclose(fi);

    float* d_cond = (float*)to_device(cond, n_cond * sizeof(float));
    float* d_x = (float*)to_device(x, n_x * sizeof(float));
    float* d_t = (float*)to_device(t, (size_t)B * sizeof(float));
    float* d_f0 = (float*)to_device(f0, n_f0 * sizeof(float));
    float *d_out = NULL, *d_wav = NULL;
    if (!d_cond || !d_x || !d_t || !d_f0 || hipMalloc((void**)&d_out, n_x * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_wav, n_wav * sizeof(float)) != hipSuccess)
        return 3;

    /* 4. cond is [B, H, T]: strides (H*T, T, 1); one backbone evaluation */
    CHECK(den, dsd_prepare_cond(den, d_cond, B, T, (int64_t)H * T, T, 1, NULL));
    CHECK(den, dsd_denoise(den, d_x, d_t, B, d_out, NULL));
    /* 5. its output [B, 1, M, T] read as a [B, num_mels, T] mel: strides (M*T, T, 1) */
    CHECK(voc, dsd_vocode(voc, d_out, B, T, (int64_t)M * T, T, 1, d_f0, NULL, NULL, NULL, d_wav, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 3;

    /* 6. both outputs */
    float* out = (float*)malloc(n_x * sizeof(float));
    float* wav = (float*)malloc(n_wav * sizeof(float));
    if (!out || !wav || hipMemcpy(out, d_out, n_x * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(wav, d_wav, n_wav * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return 3;
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    if (fwrite(out, sizeof(float), n_x, fo) != n_x || fwrite(wav, sizeof(float), n_wav, fo) != n_wav) return 2;
    fclose(fo);
    printf("wrote %zu denoised values and %zu samples\n", n_x, n_wav);
    dsd_destroy(den);
    dsd_destroy(voc);
    return 0;
}
