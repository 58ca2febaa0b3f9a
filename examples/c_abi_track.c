/*
 * A project's track from plain C: where the segments go (dsd_track_plan), each segment placed, cross-faded where it
 * overlaps what is there (dsd_track_place), the peak (dsd_track_peak) and the normalised int16 samples
 * (dsd_track_export) - the steps a C caller had to restate from the reference's inference loop after dsd_vocode_ragged.
 * No model: three synthetic segments stand in for the vocoder's output, fixed sines of different lengths laid out with
 * leading silence, one overlap (segments 0 and 1) and one gap (segments 1 and 2).  tests/test_gpu_track.py compiles this
 * with gcc, runs it on the MI355X and compares the printed total and peak and the written samples with the numpy
 * restatement of the reference's fold and save_wav.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_abi_track.c \
 *       -Ldiffsinger_amd -ldsdenoise -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/diffsinger_amd -o track
 *   ./track track.s16
 *
 * track.s16: the track as raw little-endian int16 samples at 44100 Hz, mono (WAV file writing is the caller's business).
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dsdenoise.h"

#define CHECK(call)                                                                     \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != 0) {                                                                 \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dsd_last_error(NULL));  \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

#define N_SEG 3
#define SAMPLE_RATE 44100
#define TWO_PI (2.0 * 3.14159265358979323846)

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s track.s16\n", argv[0]);
        return 2;
    }
    const int device = 0;
    const double offsets[N_SEG] = {0.010, 0.070, 0.150};           /* seconds, as a .ds project gives them */
    const int64_t lengths[N_SEG] = {3000, 2500, 1777};             /* samples, as the vocoder returns them */
    const double freq[N_SEG] = {220.0, 330.0, 440.0}, amp[N_SEG] = {0.5, 0.8, 0.3};

    /* where every segment goes: host only, before any device work */
    int64_t starts[N_SEG], prev_ends[N_SEG], total = 0;
    CHECK(dsd_track_plan(N_SEG, offsets, lengths, SAMPLE_RATE, starts, prev_ends, &total));

    /* the segments on the device (fp32, what dsd_vocode_ragged writes) */
    float* d_seg[N_SEG];
    for (int k = 0; k < N_SEG; ++k) {
        const size_t n = (size_t)lengths[k];
        float* host = (float*)malloc(n * sizeof(float));
        if (!host) return 3;
        for (size_t i = 0; i < n; ++i) host[i] = (float)(amp[k] * sin(TWO_PI * freq[k] * (double)i / (double)SAMPLE_RATE));
        if (hipMalloc((void**)&d_seg[k], n * sizeof(float)) != hipSuccess ||
            hipMemcpy(d_seg[k], host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return 3;
        free(host);
    }

    /* the track: float64, never cleared - after the last place every sample has been written */
    double *d_track = NULL, *d_peak = NULL;
    int16_t* d_pcm = NULL;
    if (hipMalloc((void**)&d_track, (size_t)total * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_peak, sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_pcm, (size_t)total * sizeof(int16_t)) != hipSuccess)
        return 3;
    for (int k = 0; k < N_SEG; ++k)                                 /* in segment order, on one stream */
        CHECK(dsd_track_place(device, d_track, total, starts[k], prev_ends[k], d_seg[k], lengths[k], NULL));
    CHECK(dsd_track_peak(device, d_track, total, d_peak, NULL));
    CHECK(dsd_track_export(device, d_track, total, DSD_TRACK_PCM, d_peak, d_pcm, NULL));   /* save_wav(norm=True) */
    if (hipDeviceSynchronize() != hipSuccess) return 3;

    double peak = 0.0;
    int16_t* pcm = (int16_t*)malloc((size_t)total * sizeof(int16_t));
    if (!pcm || hipMemcpy(&peak, d_peak, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pcm, d_pcm, (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess)
        return 3;
    FILE* fo = fopen(argv[1], "wb");
    if (!fo || fwrite(pcm, sizeof(int16_t), (size_t)total, fo) != (size_t)total) return 2;
    fclose(fo);

    long long checksum = 0;
    for (int64_t i = 0; i < total; ++i) checksum += pcm[i] < 0 ? -(long long)pcm[i] : pcm[i];
    printf("total %lld\n", (long long)total);
    printf("peak %.17g\n", peak);
    printf("checksum %lld\n", checksum);
    for (int k = 0; k < N_SEG; ++k) printf("segment%d start %lld prev_end %lld\n", k, (long long)starts[k], (long long)prev_ends[k]);

    free(pcm);
    for (int k = 0; k < N_SEG; ++k) (void)hipFree(d_seg[k]);
    (void)hipFree(d_track);
    (void)hipFree(d_peak);
    (void)hipFree(d_pcm);
    return 0;
}
