// Mel analysis: waveform -> natural-log mel spectrogram, the analysis front end the reference pairs with its vocoder
// (STFT.get_mel, modules/nsf_hifigan/nvSTFT.py:50-87, center=False).  Three launches, fp32 throughout, no FFT library:
//   mel_basis_kernel    the windowed DFT basis of one (N', W') on the device, once per size (cached by dsd_mel_analyze)
//   mel_dft_kernel      frames x basis on v_mfma_f32_16x16x4_f32 (compensated sum), reflect padding as index math while staging, |X| and the
//                       keyshift bin rule in the epilogue -> magnitudes [bin][frame] in the workspace
//   mel_project_kernel  the sparse mel projection (each filter spans a contiguous bin range), clamp, log, caller strides
// Work is listed as (item, 64-frame tile) entries, so a ragged batch computes no tile that holds only padding.
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

// ---------------------------------------------------------------------------------------------
// basis[r][j], r < Rpad, j < Kpad: row 2i = w[j] cos(2 pi k (off + j) / N), row 2i + 1 = -w[j] sin(...), k = k_lo + i, for
// the taps j < W of the periodic Hann window w[j] = 0.5 - 0.5 cos(2 pi j / W) (torch.hann_window; [1] at W = 1), which torch.stft places
// at off = (N - W) / 2 of the N-sample frame; zero elsewhere.  The phase is reduced exactly as the integer k (off + j) mod N
// before sincospif, so no fp32 angle ever exceeds 2 pi.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mel_basis_kernel(float* __restrict__ basis, int Rpad, int Kpad, int k_lo, int nb,
                                                        int N, int W, int off) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Rpad * Kpad) return;
    const int r = (int)(idx / Kpad), j = (int)(idx % Kpad), i = r >> 1;
    float v = 0.f;
    if (i < nb && j < W) {
        const long q = ((long)(k_lo + i) * (long)(off + j)) % N;
        float s, c;
        sincospif(2.f * (float)q / (float)N, &s, &c);
        const float w = W > 1 ? 0.5f - 0.5f * cospif(2.f * (float)j / (float)W) : 1.f;      // torch.hann_window(1) = [1.]
        v = (r & 1) ? -(w * s) : w * c;
    }
    basis[idx] = v;
}

// ---------------------------------------------------------------------------------------------
// One workgroup = one (item, 64-frame tile) entry x one 64-row tile of the basis, through dft_tile_walk (dsd_device.h):
// accumulator registers 0 / 1 hold the re / im rows of one bin and 2 / 3 those of the next, so the magnitude needs no lane
// movement.  Frame t of item b reads padded sample t H + off + j, i.e. sample i = t H + off + j - padL of the item,
// reflected at both ends of its own length L (torch's reflect pad: -i, 2 (L - 1) - i); a ragged item never reads past its end.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mel_dft_kernel(const MelDftP p) {
    __shared__ float sA[kDftRows * kDftLS];
    __shared__ float sB[kDftFrames * kDftLS];
    const int* e = p.work + 5 * blockIdx.x;
    const int b = e[0], t0 = e[1], L = e[2], Tb = e[3], g0 = e[4];
    const int rt = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* __restrict__ x = p.wav + (long)b * p.wav_bstride;
    f32x4 hi[4], lo[4];
    dft_tile_walk(p.basis + (long)rt * kDftRows * p.Kpad, p.Kpad, p.W, Tb - t0, sA, sB, [&](int f, int j) {
        long i = (long)(t0 + f) * p.H + p.off + j - p.padL;
        if (i < 0) i = -i;
        if (i >= L) i = 2 * (long)(L - 1) - i;
        return x[i];
    }, hi, lo);
    // epilogue: |X| (nvSTFT.py:69-74 .abs()), then with a key shift * win_size / W' in torch's order (nvSTFT.py:80)
    const int bin0 = rt * (kDftRows / 2) + 8 * w + 2 * (lane >> 4);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int fr = 16 * f + (lane & 15);
        if (t0 + fr >= Tb) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int bin = bin0 + h;
            if (bin >= p.nb) continue;
            const float re = hi[f][2 * h] + lo[f][2 * h], im = hi[f][2 * h + 1] + lo[f][2 * h + 1];
            float m = sqrtf(re * re + im * im);
            if (p.rescale) m = (m * p.win_size) / p.win_new;
            p.mags[(long)bin * p.G + g0 + fr] = m;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// mel[m] = log(max(sum_{k in [lo_m, hi_m)} fb[m][k] |X[k]|, clip))  (nvSTFT.py:82-85): the filterbank's non-zero run of each
// filter, packed; ranges are bin indices relative to k_lo and clipped to the bins this call computed (nb).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mel_project_kernel(const MelProjP p) {
    const int* e = p.work + 5 * blockIdx.x;
    const int b = e[0], t0 = e[1], Tb = e[3], g0 = e[4];
    for (int idx = threadIdx.x; idx < kDftFrames * p.M; idx += 256) {
        const int f = idx % kDftFrames, m = idx / kDftFrames, t = t0 + f;
        if (t >= Tb) continue;
        const int lo = p.range[2 * m], hi = min(p.range[2 * m + 1], p.nb), woff = p.woff[m];
        float s = 0.f;
        for (int k = lo; k < hi; ++k) s = fmaf(p.fw[woff + k - lo], p.mags[(long)k * p.G + g0 + f], s);
        // the logarithm in double, rounded once: the device's logf is up to 2 ulp off (1.9e-6 at log(1e-5), which every
        // clamped entry holds; 8e-7 of the peak mel, linear, where the peak is ~1e-4), the reference's CPU log within 1
        p.out[(long)b * p.o_sb + (long)m * p.o_sm + (long)t * p.o_st] = (float)log((double)fmaxf(s, p.clip));
    }
}

hipError_t launch_mel_basis(float* basis, int Rpad, int Kpad, int k_lo, int nb, int N, int W, int off, hipStream_t st) {
    const long n = (long)Rpad * Kpad;
    hipLaunchKernelGGL(mel_basis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, basis, Rpad, Kpad, k_lo, nb,
                       N, W, off);
    return hipGetLastError();
}

hipError_t launch_mel_dft(const MelDftP& p, int n_entries, int row_tiles, hipStream_t st) {
    hipLaunchKernelGGL(mel_dft_kernel, dim3((unsigned)n_entries, (unsigned)row_tiles), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_mel_project(const MelProjP& p, int n_entries, hipStream_t st) {
    hipLaunchKernelGGL(mel_project_kernel, dim3((unsigned)n_entries), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace dsd
