// VR harmonic-noise separation (modules/hnsep/vr/: CascadedNet.predict_from_audio, is_complex=True) and the variance curves
// built on it (utils/binarizer_utils.py: get_energy_librosa, get_breathiness, get_voicing, get_tension_base_harmonic;
// utils/decomposed_waveform.py: _kth_harmonic(0)), fp32 throughout:
//   hs_basis_kernel   the windowed DFT basis (forward: [2 bins][taps]) or the windowed inverse basis ([taps][2 bins]) on the
//                     device, from a host window
//   hs_dft_kernel     forward: frames x basis on v_mfma_f32_16x16x4_f32 (compensated sum), zero or reflect padding as index
//                     math while staging -> the complex spectrogram in the network's layout; inverse: the masked spectrum
//                     (the network's complex mask or the f0 bin mask applied while staging) x the inverse basis -> windowed
//                     frames
//   hs_ola_kernel     overlap-add of the frames, the window-square envelope division and the crop, one pass (the mean of the
//                     channels of a stereo model)
//   hs_conv_kernel    2-D conv as an implicit GEMM on v_mfma_f32_16x16x4_f32: 3x3 (stride 1 / 2, per-axis dilation) or 1x1,
//                     BN folded into the weights and the shift, ReLU / LeakyReLU in the epilogue; reads a concat of up to
//                     four sources, each plain, bilinear x2 (align_corners) upsampled while staging, or broadcast over bins
//   hs_binmean_kernel the ASPP's mean over bins
//   hs_lstm_kernel    one LSTM direction of one sub-net and item per workgroup, W_hh in LDS
//   hs_mask_kernel    bounded_mask of the `out` conv
//   hs_rms_kernel / hs_curves_kernel   framed RMS of the four signals, then per item: pad / crop, dB with the top-db clamp,
//                     the tension domains
// Activations are [item][bin][frame][channel] (channels innermost) with caller-described strides, so a view into a
// concatenation over bins or channels is a pointer and strides.  Work is listed per (item, tile) with the item's own padded
// frame count, so a ragged item computes exactly as its lone call.
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

// ---------------------------------------------------------------------------------------------
// Forward (inv = 0): basis[r][j], r < Rpad, j < Kpad: row 2i = w[j] cos(2 pi i j / N), row 2i + 1 = -w[j] sin(...), i < nb.
// Inverse (inv = 1): basis[j][r], j < Rpad (samples), r < Kpad: column 2i = a_i w[j] cos(2 pi i j / N) / N, column 2i + 1 =
// -a_i w[j] sin(...) / N, a_0 = a_{N/2} = 1, else 2 (irfft: the imaginary parts of DC and Nyquist drop out as sin = 0).
// The phase is reduced as the integer i j mod N before sincospif.  (Kept apart from mel_basis_kernel, which computes its
// Hann window on the device in fp32 with cospif: one kernel for both would change bits.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hs_basis_kernel(float* __restrict__ basis, const float* __restrict__ win, int Rpad,
                                                       int Kpad, int nb, int N, int inv) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Rpad * Kpad) return;
    const int row = (int)(idx / Kpad), col = (int)(idx % Kpad);
    const int r = inv ? col : row, j = inv ? row : col, i = r >> 1;
    float v = 0.f;
    if (i < nb && j < N) {
        const long q = ((long)i * (long)j) % N;
        float s, c;
        sincospif(2.f * (float)q / (float)N, &s, &c);
        const float w = win[j];
        if (inv) {
            const float a = (i == 0 || 2 * i == N) ? 1.f : 2.f;
            v = (r & 1) ? -(a * w * s) / (float)N : (a * w * c) / (float)N;
        } else {
            v = (r & 1) ? -(w * s) : w * c;
        }
    }
    basis[idx] = v;
}

// ---------------------------------------------------------------------------------------------
// One workgroup = one (item, 64-frame tile, channel) entry x one 64-row tile of the basis, through dft_tile_walk
// (dsd_device.h).  work: (b, t0, L, T_b, ch, padL).
// Forward (INV = 0): frame t reads sample t H + j - padL of channel ch of the item (L samples), zero (pad_mode 'constant')
// or reflected (torch's 'reflect') outside; accumulator registers 0 / 1 (2 / 3) are re / im of one bin, written to channels
// [c] / [s_cim + c], ch <= c < ch + nrep (nrep > 1: one clip repeated to every channel, wav_sc = 0).
// Inverse (INV = 1): frame t's K = 2 nb vector is (re, im) of the spectrum times the mask: the network's complex mask [bin min(i, mask_F - 1)]
// (replicate pad), or the
// f0 bin mask of _kth_harmonic (frames t >= f0 frames: 0); rows are samples j -> frames buffer.
// ---------------------------------------------------------------------------------------------
template <int INV>
__global__ __launch_bounds__(256) void hs_dft_kernel(const std::conditional_t<INV, HsIstftP, HsStftP> p) {
    __shared__ float sA[kDftRows * kDftLS];
    __shared__ float sB[kDftFrames * kDftLS];
    const int* e = p.work + 6 * blockIdx.x;
    const int b = e[0], t0 = e[1], Tb = e[3], ch = e[4];
    const int rt = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    f32x4 hi[4], lo[4];
    if constexpr (!INV) {
        const int L = e[2], padL = e[5];
        dft_tile_walk(p.basis + (long)rt * kDftRows * p.N, p.N, p.N, Tb - t0, sA, sB, [&](int f, int j) {
            long i = (long)(t0 + f) * p.H + j - padL;
            if (p.reflect) {
                if (i < 0) i = -i;
                if (i >= L) i = 2 * (long)(L - 1) - i;
            }
            return i >= 0 && i < L ? p.wav[(long)b * p.wav_sb + (long)ch * p.wav_sc + i] : 0.f;
        }, hi, lo);
        const int bin0 = rt * (kDftRows / 2) + 8 * w + 2 * (lane >> 4);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int t = t0 + 16 * f + (lane & 15);
            if (t >= Tb) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int bin = bin0 + h;
                if (bin >= p.nb) continue;
                float* o = p.spec + (long)b * p.s_sb + (long)bin * p.s_sf + (long)t * p.s_st;
                const float re = hi[f][2 * h] + lo[f][2 * h], im = hi[f][2 * h + 1] + lo[f][2 * h + 1];
                for (int c = ch; c < ch + p.nrep; ++c) {
                    o[c] = re;
                    o[p.s_cim + c] = im;
                }
            }
        }
    } else {
        dft_tile_walk(p.basis + (long)rt * kDftRows * p.Kpad, p.Kpad, 2 * p.nb, Tb - t0, sA, sB, [&](int f, int j) {
            const int t = t0 + f, bin = j >> 1;
            const float* sp = p.spec + (long)b * p.s_sb + (long)bin * p.s_sf + (long)t * p.s_st;
            const float sr = sp[ch], si = sp[p.s_cim + ch];
            float mr, mi;
            if (p.mask) {
                const float* mp = p.mask + (long)b * p.m_sb + (long)min(bin, p.mask_F - 1) * p.m_sf + (long)t * p.m_st;
                mr = mp[ch];
                mi = mp[p.m_cim + ch];
            } else {        // _kth_harmonic: center = f0 win / sr, [max(center - hw, 0), min(center + hw, n_specs))
                const float f0 = t < p.f0_len[b] ? p.f0[(long)b * p.f0_sb + t] : 0.f;
                const float center = f0 * (float)p.N / p.sr;
                const float st = fmaxf(center - p.half_width, 0.f), en = fminf(center + p.half_width, (float)p.nb);
                const float fb = (float)bin;
                mr = (t < p.f0_len[b] && center >= 1.f && fb >= st && fb < en) ? 1.f : 0.f;
                mi = 0.f;
            }
            return (j & 1) ? sr * mi + si * mr : sr * mr - si * mi;
        }, hi, lo);
        const int row0 = rt * kDftRows + 16 * w + 4 * (lane >> 4);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int t = t0 + 16 * f + (lane & 15);
            if (t >= Tb) continue;
            float* o = p.frames + ((long)(b * p.nch + ch) * p.f_sb) + (long)t * p.N;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < p.N) o[row0 + r] = hi[f][r] + lo[f][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// torch.istft's overlap-add: padded position q = n + off0 of output sample n sums frames t with 0 <= q - t H < N,
// t < T_b, then divides by the same sum of w^2; the channels of one item are written apart (o_sc != 0) or averaged
// ((y0 + y1) / 2, torch.mean: DecomposedWaveformVocalRemover._infer).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hs_ola_kernel(const HsOlaP p) {
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= p.len[b]) return;
    const long q = n + p.off0[b];
    const int Tb = p.T[b];
    const long th = min((long)Tb - 1, q / p.H);
    const long tl = q - (p.N - 1) <= 0 ? 0 : (q - (p.N - 1) + p.H - 1) / p.H;
    float env = 0.f;
    for (long t = tl; t <= th; ++t) {
        const float wv = p.win[q - t * p.H];
        env += wv * wv;
    }
    float acc = 0.f;
    for (int c = 0; c < p.nch; ++c) {
        const float* fr = p.frames + (long)(b * p.nch + c) * p.f_sb;
        float y = 0.f;
        for (long t = tl; t <= th; ++t) y += fr[t * p.N + q - t * p.H];
        if (p.o_sc) p.out[(long)b * p.o_sb + (long)c * p.o_sc + n] = y / env;
        acc += y / env;
    }
    if (!p.o_sc) p.out[(long)b * p.o_sb + n] = p.nch == 1 ? acc : acc / (float)p.nch;
}

// ---------------------------------------------------------------------------------------------
// Conv as an implicit GEMM: M = output positions (16 per wave, 64 per workgroup), N = output channels (NB blocks of 16 per
// wave; blockIdx.y = the channel group), K = (source, tap, channel) with each source's channels padded to 4 (the K step).
// Position q < F T_l of the item: bin q / T_l, frame q % T_l.  Tap (kf, kt) reads input (f s - pad + kf d_f, t s - pad + kt d_t)
// of the conv's input grid (F_in x T_in; zero outside).  Source modes: 0 plain; 1 the bilinear x2 upsample (align_corners)
// of a (F_in / 2) x (T_in / 2) tensor, computed while staging (torch's upsample_bilinear2d: scale (in - 1) / (out - 1),
// lambda = src - floor(src), neighbour clamped); 2 one bin broadcast over all bins.  work: (b, q0, T_l out, T_l in).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float hs_src_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

template <int NB>
__global__ __launch_bounds__(256) void hs_conv_kernel(const HsConvP p) {
    const int* e = p.work + 4 * blockIdx.x;
    const int b = e[0], Tl = e[2], Tin = e[3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, kq = lane >> 4, li = lane & 15;
    const int npos = p.F * Tl;
    const int qa = e[1] + 16 * w + li;                       // this lane's A-operand position
    const int qc = min(qa, npos - 1);
    const int fo = qc / Tl, to = qc % Tl;
    const int co0 = blockIdx.y * 16 * NB;
    const int pad_f = p.ks == 3 ? p.dil_f : 0, pad_t = p.ks == 3 ? p.dil_t : 0;
    f32x4 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ wrow = p.w + co0 + li;
    int kb = 0;
    for (int s = 0; s < p.nsrc; ++s) {
        const HsSrc& S = p.src[s];
        const float* __restrict__ sp = S.p + (long)b * S.bs;
        const int Fs = S.mode == 1 ? p.Fin >> 1 : p.Fin, Ts = S.mode == 1 ? Tin >> 1 : Tin;
        const float scf = hs_src_scale(Fs, p.Fin), sct = hs_src_scale(Ts, Tin);
        for (int kf = 0; kf < p.ks; ++kf)
            for (int kt = 0; kt < p.ks; ++kt) {
                const int fi = fo * p.stride - pad_f + kf * p.dil_f, ti = to * p.stride - pad_t + kt * p.dil_t;
                const bool in = fi >= 0 && fi < p.Fin && ti >= 0 && ti < Tin;
                long o00 = 0, o01 = 0, o10 = 0, o11 = 0;
                float h0l = 1.f, h1l = 0.f, w0l = 1.f, w1l = 0.f;
                if (in) {
                    if (S.mode == 0) {
                        o00 = (long)fi * S.fs + (long)ti * S.ts;
                    } else if (S.mode == 2) {
                        o00 = (long)ti * S.ts;
                    } else {
                        const float hr = scf * (float)fi, wr = sct * (float)ti;
                        const int h0 = (int)hr, w0 = (int)wr;
                        const int hp = h0 < Fs - 1 ? 1 : 0, wp = w0 < Ts - 1 ? 1 : 0;
                        h1l = hr - (float)h0;
                        h0l = 1.f - h1l;
                        w1l = wr - (float)w0;
                        w0l = 1.f - w1l;
                        o00 = (long)h0 * S.fs + (long)w0 * S.ts;
                        o01 = o00 + wp * S.ts;
                        o10 = o00 + hp * S.fs;
                        o11 = o10 + wp * S.ts;
                    }
                }
                // one tap's channels sum into a fresh accumulator, the taps' partial sums into acc: at nout 64 a conv's K
                // reaches 8064, and 2016 MFMA steps into one fp32 accumulator left the harmonic part 2.1e-6 from the float64
                // oracle where the blocked sums of the reference's CPU path are 5e-7 from it
                f32x4 part[NB];
#pragma unroll
                for (int n = 0; n < NB; ++n) part[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int c0 = 0; c0 < S.Cp; c0 += 4) {
                    const int c = c0 + kq;
                    float a = 0.f;
                    if (in && c < S.C) {
                        const float* x = sp + (long)c * S.cs;
                        if (S.mode == 1)
                            a = h0l * (w0l * x[o00] + w1l * x[o01]) + h1l * (w0l * x[o10] + w1l * x[o11]);
                        else
                            a = x[o00];
                    }
                    const float* __restrict__ wk = wrow + (long)(kb + c) * p.cout_pad;
#pragma unroll
                    for (int n = 0; n < NB; ++n) part[n] = mfma_16x16x4(a, wk[16 * n], part[n]);
                }
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[n] += part[n];
                kb += S.Cp;
            }
    }
    // epilogue: D[position 4 kq + r][channel li] of each 16-channel block
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int co = co0 + 16 * n + li;
        if (co >= p.cout) continue;
        const float sh = p.shift[co];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = e[1] + 16 * w + 4 * kq + r;
            if (q >= npos) continue;
            float v = acc[n][r] + sh;
            if (p.act == 1) v = fmaxf(v, 0.f);
            else if (p.act == 2) v = v < 0.f ? v * 0.01f : v;
            const int f = q / Tl, t = q % Tl;
            p.y.p[(long)b * p.y.bs + (long)f * p.y.fs + (long)t * p.y.ts + (long)co * p.y.cs] = v;
        }
    }
}

// y[b][0][t][c] = mean over the F bins of x[b][f][t][c] (ASPPModule's Mean(dim=-2)), t < T_b
__global__ __launch_bounds__(256) void hs_binmean_kernel(const HsBinMeanP p) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)(idx / p.C), c = (int)(idx % p.C);
    if (t >= p.T[b]) return;
    const float* x = p.x.p + (long)b * p.x.bs + (long)t * p.x.ts + (long)c * p.x.cs;
    float s = 0.f;
    for (int f = 0; f < p.F; ++f) s += x[(long)f * p.x.fs];
    p.y.p[(long)b * p.y.bs + (long)t * p.y.ts + (long)c * p.y.cs] = s / (float)p.F;
}

// ---------------------------------------------------------------------------------------------
// blockIdx = (item, sub-net, direction).  Thread r < 4H owns gate row r (order i, f, g, o) of W_hh, which sits in LDS as
// [k][4H] (conflict-free column reads).  Per step: g = gi[t] + W_hh h (gi holds x W_ih^T + b_ih + b_hh), then unit j < H:
//   c' = s(g_f) c + s(g_i) tanh(g_g), h' = s(g_o) tanh(c')          (torch.nn.LSTM)
// The item runs over its own T_b frames; the reverse direction starts at T_b - 1.  gi: [b][t][2 4H] (forward | reverse),
// y: [b][t][2H] (forward | reverse h).
// ---------------------------------------------------------------------------------------------
constexpr int HS_HMAX = 64;
__global__ __launch_bounds__(4 * HS_HMAX) void hs_lstm_kernel(const HsLstmP p) {
    __shared__ float sW[HS_HMAX * 4 * HS_HMAX];
    __shared__ float sh[HS_HMAX];
    __shared__ float sg[4 * HS_HMAX];
    const int b = blockIdx.x, d = blockIdx.z, r = threadIdx.x;
    const HsLstmNet& net = p.net[blockIdx.y];
    const int H = net.H, G = 4 * H, Tb = p.T[b];
    const float* __restrict__ whh = net.whh + (long)d * G * H;        // [4H][H] of direction d
    for (int idx = r; idx < G * H; idx += blockDim.x) {
        const int row = idx / H, k = idx % H;
        sW[k * G + row] = whh[idx];
    }
    if (r < H) sh[r] = 0.f;
    float c = 0.f;
    __syncthreads();
    for (int s = 0; s < Tb; ++s) {
        const int t = d ? Tb - 1 - s : s;
        if (r < G) {
            float a0 = 0.f, a1 = 0.f;
            for (int k = 0; k < H; k += 2) {
                a0 = fmaf(sW[k * G + r], sh[k], a0);
                a1 = fmaf(sW[(k + 1) * G + r], sh[k + 1], a1);
            }
            sg[r] = net.gi[(long)b * net.gi_bs + (long)t * 2 * G + d * G + r] + (a0 + a1);
        }
        __syncthreads();
        if (r < H) {
            const float ig = 1.f / (1.f + expf(-sg[r]));
            const float fg = 1.f / (1.f + expf(-sg[H + r]));
            const float gg = tanhf(sg[2 * H + r]);
            const float og = 1.f / (1.f + expf(-sg[3 * H + r]));
            c = fmaf(fg, c, ig * gg);
            const float hn = og * tanhf(c);
            sh[r] = hn;
            net.y[(long)b * net.y_bs + (long)t * 2 * H + d * H + r] = hn;
        }
        __syncthreads();
    }
}

// bounded_mask: m = (re, im) of the `out` conv at (b, min(f, Fx - 1), t) (the replicate pad to F bins),
// tanh(|m|) m / (|m| + 1e-8) -> channel c of the mask: re at c cs, im at y_im + c cs
__global__ __launch_bounds__(256) void hs_mask_kernel(const HsMaskP p) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int Tb = p.T[b];
    if (idx >= (long)p.F * Tb * p.C) return;
    const int c = (int)(idx % p.C), t = (int)((idx / p.C) % Tb), f = (int)(idx / ((long)p.C * Tb));
    const float* x = p.x.p + (long)b * p.x.bs + (long)min(f, p.Fx - 1) * p.x.fs + (long)t * p.x.ts;
    const float re = x[c * p.x.cs], im = x[(p.C + c) * p.x.cs];
    const float mag = sqrtf(re * re + im * im), th = tanhf(mag);
    float* y = p.y.p + (long)b * p.y.bs + (long)f * p.y.fs + (long)t * p.y.ts + (long)c * p.y.cs;
    y[0] = th * re / (mag + 1e-8f);
    y[p.y_im] = th * im / (mag + 1e-8f);
}

// ---------------------------------------------------------------------------------------------
// librosa 0.9.2 feature.rms(y, frame_length=win, hop_length=hop, center=True, pad_mode="constant"): frame t of the item's
// L samples covers [t hop - win / 2, t hop + win / 2), zero outside; rms = sqrt(mean(y^2)), summed in double.  One thread =
// (item, frame) x the four signals: the waveform, the aperiodic part (waveform - harmonic, in fp32), the harmonic part,
// the base harmonic (each optional).  rms: [4][b][Tmax]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hs_rms_kernel(const HsRmsP p) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const long L = p.len[b];
    if (t >= p.nfr[b]) return;
    const float* x = p.wav ? p.wav + (long)b * p.sb : nullptr;
    const float* h = p.harm ? p.harm + (long)b * p.sb : nullptr;
    const float* g = p.base ? p.base + (long)b * p.sb : nullptr;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const long i0 = (long)t * p.hop - p.win / 2;
    for (int j = 0; j < p.win; ++j) {
        const long i = i0 + j;
        if (i < 0 || i >= L) continue;
        const float xv = x ? x[i] : 0.f, hv = h ? h[i] : 0.f, gv = g ? g[i] : 0.f, av = xv - hv;
        s[0] += (double)xv * xv;
        s[1] += (double)av * av;
        s[2] += (double)hv * hv;
        s[3] += (double)gv * gv;
    }
    for (int k = 0; k < 4; ++k) p.rms[((long)k * p.B + b) * p.Tmax + t] = (float)sqrt(s[k] / p.win);
}

// amplitude_to_db(a, ref=1, amin=1e-5, top_db=80) after the pad / crop to `length` frames: max(10 log10(max(1e-10, a^2)),
// item max - 80).  One workgroup per item.  Tension (binarizer_utils.py:200-208): sqrt(clip(E_h^2 - E_b^2, 0)) / (E_h + 1e-5),
// domain 0 'ratio' (clip [0, 1]), 1 'db' (clip [1e-5, 1], dB), 2 'logit' (clip [1e-4, 1 - 1e-4], log(x / (1 - x))).
__device__ float hs_db_pass(float* __restrict__ y, int n, float* red) {
    float m = -INFINITY;
    for (int t = threadIdx.x; t < n; t += 256) {
        const float a = y[t];
        const float v = 10.f * log10f(fmaxf(1e-10f, a * a));
        y[t] = v;
        m = fmaxf(m, v);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float floor_db = red[0] - 80.f;
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += 256) y[t] = fmaxf(y[t], floor_db);
    return floor_db;
}

__global__ __launch_bounds__(256) void hs_curves_kernel(const HsCurvesP p) {
    __shared__ float red[256];
    const int b = blockIdx.x, n = p.length[b], nf = p.nfr[b];
    auto rms = [&](int k, int t) { return t < nf ? p.rms[((long)k * p.B + b) * p.Tmax + t] : 0.f; };
    for (int k = 0; k < 3; ++k) {               // energy (waveform), breathiness (aperiodic), voicing (harmonic)
        float* y = p.out[k];
        if (!y) continue;
        y += (long)b * p.o_sb;
        for (int t = threadIdx.x; t < n; t += 256) y[t] = rms(k, t);
        __syncthreads();
        if (p.db) hs_db_pass(y, n, red);
        __syncthreads();
    }
    float* y = p.out[3];
    if (!y) return;
    y += (long)b * p.o_sb;
    for (int t = threadIdx.x; t < n; t += 256) {
        const float eh = rms(2, t), eb = rms(3, t);
        float v = sqrtf(fmaxf(eh * eh - eb * eb, 0.f)) / (eh + 1e-5f);
        if (p.domain == 0) v = fminf(fmaxf(v, 0.f), 1.f);
        else if (p.domain == 1) v = fminf(fmaxf(v, 1e-5f), 1.f);
        else {
            v = fminf(fmaxf(v, 1e-4f), 1.f - 1e-4f);
            v = logf(v / (1.f - v));
        }
        y[t] = v;
    }
    __syncthreads();
    if (p.domain == 1) hs_db_pass(y, n, red);
}

hipError_t launch_hs_basis(float* basis, const float* win, int Rpad, int Kpad, int nb, int N, int inv, hipStream_t st) {
    const long n = (long)Rpad * Kpad;
    hipLaunchKernelGGL(hs_basis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, basis, win, Rpad, Kpad, nb, N, inv);
    return hipGetLastError();
}
hipError_t launch_hs_stft(const HsStftP& p, int n_entries, int row_tiles, hipStream_t st) {
    hipLaunchKernelGGL(hs_dft_kernel<0>, dim3((unsigned)n_entries, (unsigned)row_tiles), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_istft(const HsIstftP& p, int n_entries, int row_tiles, hipStream_t st) {
    hipLaunchKernelGGL(hs_dft_kernel<1>, dim3((unsigned)n_entries, (unsigned)row_tiles), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_ola(const HsOlaP& p, int B, long max_len, hipStream_t st) {
    hipLaunchKernelGGL(hs_ola_kernel, dim3((unsigned)((max_len + 255) / 256), (unsigned)B), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_conv(const HsConvP& p, int n_entries, hipStream_t st) {
    const int nblk = p.cout_pad / 16;
    const int NB = nblk % 8 == 0 ? 8 : nblk % 4 == 0 ? 4 : nblk % 2 == 0 ? 2 : 1;
    const dim3 grid((unsigned)n_entries, (unsigned)(nblk / NB));
    switch (NB) {
        case 8: hipLaunchKernelGGL(hs_conv_kernel<8>, grid, dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL(hs_conv_kernel<4>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(hs_conv_kernel<2>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(hs_conv_kernel<1>, grid, dim3(256), 0, st, p); break;
    }
    return hipGetLastError();
}
hipError_t launch_hs_binmean(const HsBinMeanP& p, int B, int Tmax, hipStream_t st) {
    const long n = (long)Tmax * p.C;
    hipLaunchKernelGGL(hs_binmean_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_lstm(const HsLstmP& p, int B, int nnet, hipStream_t st) {
    hipLaunchKernelGGL(hs_lstm_kernel, dim3((unsigned)B, (unsigned)nnet, 2), dim3(4 * HS_HMAX), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_mask(const HsMaskP& p, int B, int Tmax, hipStream_t st) {
    const long n = (long)p.F * Tmax * p.C;
    hipLaunchKernelGGL(hs_mask_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_rms(const HsRmsP& p, hipStream_t st) {
    hipLaunchKernelGGL(hs_rms_kernel, dim3((unsigned)((p.Tmax + 255) / 256), (unsigned)p.B), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_hs_curves(const HsCurvesP& p, hipStream_t st) {
    hipLaunchKernelGGL(hs_curves_kernel, dim3((unsigned)p.B), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace dsd
