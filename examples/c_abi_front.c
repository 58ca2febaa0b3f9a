/*
 * A segment's front end from plain C: its phoneme durations in seconds to frame counts (dsd_seconds_to_frames - host
 * arithmetic, so T is known before anything is on the device), the frame counts to mel2ph (dsd_length_regulate), and three
 * of its control curves - f0 as MIDI pitch with the unvoiced frames filled, an energy curve, a velocity curve clipped to
 * the model's range - to the model's frame rate in one dsd_curve_resample call: the steps a C caller had to restate from
 * the reference's inference/ds_acoustic.py and utils/infer_utils.py before the first encoder call.
 * No model: the segment is synthetic.  tests/test_gpu_front.py compiles this with gcc, runs it on the MI355X and compares
 * the written arrays with the numpy restatement of the reference.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_front.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/diffsinger_amd -o front
 *   ./front front.bin
 *
 * front.bin: int64 T, int64 mel2ph[T], then fp32 pitch[T], energy[T], speed[T] and T bytes of uv.
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
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dsd_last_error(NULL));  \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

#define N_PH 7
#define N_F0 461
#define N_ENERGY 231
#define N_VELOCITY 24

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s front.bin\n", argv[0]);
        return 2;
    }
    const int device = 0;
    const double timestep = 512.0 / 44100.0;                        /* hop_size / audio_sample_rate */
    const float ph_dur[N_PH] = {0.12f, 0.305f, 0.0f, 0.61f, 0.2175f, 0.48f, 0.57f};   /* seconds, as a .ds segment gives them */

    /* frames per phoneme and the segment's frame count: host only */
    int64_t frames[N_PH], T = 0;
    CHECK(dsd_seconds_to_frames(ph_dur, N_PH, timestep, frames, &T));

    /* the curves as the segment carries them: f0 every 5 ms with an unvoiced head, gap and tail; energy every 10 ms;
     * velocity every 100 ms, reaching past both bounds of [0.5, 2] */
    const int n_pts[3] = {N_F0, N_ENERGY, N_VELOCITY};
    const double steps[3] = {0.005, 0.01, 0.1};
    float* host = (float*)malloc((N_F0 + N_ENERGY + N_VELOCITY) * sizeof(float));
    if (!host) return 3;
    for (int i = 0; i < N_F0; ++i)
        host[i] = (i < 9 || (i >= 200 && i < 262) || i >= 440) ? 0.f : 220.f + 0.25f * (float)((i * 37) % 401);
    for (int i = 0; i < N_ENERGY; ++i) host[N_F0 + i] = -60.f + 0.125f * (float)((i * 53) % 397);
    for (int i = 0; i < N_VELOCITY; ++i) host[N_F0 + N_ENERGY + i] = 0.25f + 0.125f * (float)((i * 7) % 20);

    float *d_pts = NULL, *d_out = NULL;
    uint8_t* d_uv = NULL;
    int64_t *d_dur = NULL, *d_mel2ph = NULL;
    const size_t n_all = N_F0 + N_ENERGY + N_VELOCITY;
    if (hipMalloc((void**)&d_pts, n_all * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_out, 3 * (size_t)T * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_uv, (size_t)T) != hipSuccess ||
        hipMalloc((void**)&d_dur, N_PH * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void**)&d_mel2ph, (size_t)T * sizeof(int64_t)) != hipSuccess ||
        hipMemcpy(d_pts, host, n_all * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_dur, frames, N_PH * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
        return 3;

    CHECK(dsd_length_regulate(device, d_dur, 1, N_PH, (int32_t)T, d_mel2ph, NULL));

    dsd_curve curves[3];
    memset(curves, 0, sizeof(curves));
    size_t off = 0;
    for (int k = 0; k < 3; ++k) {
        curves[k].points = d_pts + off;
        curves[k].out = d_out + (size_t)k * (size_t)T;
        curves[k].src_step = steps[k];
        curves[k].dst_step = timestep;
        curves[k].n_points = n_pts[k];
        curves[k].length = (int32_t)T;
        curves[k].pad_to = (int32_t)T;
        off += (size_t)n_pts[k];
    }
    curves[0].op = DSD_CURVE_PITCH;
    curves[0].uv_out = d_uv;
    curves[1].op = DSD_CURVE_PLAIN;
    curves[2].op = DSD_CURVE_CLIP;
    curves[2].lo = 0.5f;
    curves[2].hi = 2.0f;
    CHECK(dsd_curve_resample(device, curves, 3, NULL));
    if (hipDeviceSynchronize() != hipSuccess) return 3;

    int64_t* mel2ph = (int64_t*)malloc((size_t)T * sizeof(int64_t));
    float* out = (float*)malloc(3 * (size_t)T * sizeof(float));
    uint8_t* uv = (uint8_t*)malloc((size_t)T);
    if (!mel2ph || !out || !uv ||
        hipMemcpy(mel2ph, d_mel2ph, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out, d_out, 3 * (size_t)T * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(uv, d_uv, (size_t)T, hipMemcpyDeviceToHost) != hipSuccess)
        return 3;
    FILE* fo = fopen(argv[1], "wb");
    if (!fo || fwrite(&T, sizeof(T), 1, fo) != 1 || fwrite(mel2ph, sizeof(int64_t), (size_t)T, fo) != (size_t)T ||
        fwrite(out, sizeof(float), 3 * (size_t)T, fo) != 3 * (size_t)T || fwrite(uv, 1, (size_t)T, fo) != (size_t)T)
        return 2;
    fclose(fo);

    printf("frames");
    for (int i = 0; i < N_PH; ++i) printf(" %lld", (long long)frames[i]);
    printf("\ntotal %lld\n", (long long)T);

    free(host); free(mel2ph); free(out); free(uv);
    (void)hipFree(d_pts); (void)hipFree(d_out); (void)hipFree(d_uv); (void)hipFree(d_dur); (void)hipFree(d_mel2ph);
    return 0;
}
