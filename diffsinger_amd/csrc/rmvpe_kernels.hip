// RMVPE pitch extraction (modules/pe/rmvpe/, E2E0 + MelSpectrogram + to_local_average_f0 / to_viterbi_f0), fp32 throughout
// but for the Viterbi recursion, which is double:
//   rm_resample_kernel  torchaudio's sinc_interp_hann Resample(sr, 16000, lowpass_filter_width=128) as a polyphase FIR
//   rm_prep_kernel      log-mel [b][m][t] (caller strides) -> unet.encoder.bn(pad(mel)) in the [b][t][f] layout
//   rm_conv3_kernel     3x3 conv (BN folded into the weights) + ReLU, then the ConvBlockRes residual (identity or the 1x1
//                       shortcut conv), optionally the AvgPool2d(2) of the result; reads two sources as one concat
//   rm_tconv_kernel     ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1) + folded BN + ReLU
//   rm_linear_kernel    frames x weights (+ bias, optional sigmoid): the GRU input projections and the Linear heads
//   rm_gru_kernel       one GRU direction of one item per workgroup; W_hh split over registers, LDS and L2
//   rm_decode_kernel    argmax (or a given centre), the local weighted average of the cents, f0, the threshold
//   rm_logprob_kernel, rm_viterbi_kernel   to_viterbi_f0's path (librosa.sequence.viterbi) in double: the centres of the decode
// Activations are [item][frame][bin][channel] (channels innermost): the K walk of a conv is contiguous in the channels,
// and the head's [frame][bin][3] output is the GRU's input row as it stands.
// Work is listed per (item, tile) with the item's own frame count, so a ragged item computes exactly as its lone call.
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

constexpr int RM_CO = 8;            // output channels per thread (conv / tconv), outputs per thread (linear)

// ---------------------------------------------------------------------------------------------
// out[b][blk * nw + ph] = sum_k kern[ph][k] xpad[blk * orig + k], xpad = the item's samples behind `width` zeros, zeros past
// its end (_apply_sinc_resample_kernel: pad (width, width + orig), conv1d stride orig, phases interleaved).  blockIdx.y =
// phase: the kernel row is wave-uniform.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_resample_kernel(const RmResampleP p) {
    const int b = blockIdx.z, ph = blockIdx.y;
    const long blk = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = blk * p.nw + ph, L = p.len_in[b];
    if (i >= p.len_out[b]) return;
    const float* __restrict__ x = p.x + (long)b * p.x_sb;
    const float* __restrict__ kr = p.kern + (long)ph * p.K;
    const long j0 = blk * p.orig - p.width;
    float out;
    if (p.nw > p.orig) {
        // upsampling (nw > orig: every rate below 16 kHz; measured at 8 kHz): the bands above the input's Nyquist hold the
        // filter's stop band alone, next to the log-mel's clamp, and there the 5e-7 of a sequential fp32 sum is what the
        // network sees (2.4e-6 in the hidden): summed in double and rounded once.  Downsampling fills the whole band and
        // keeps the fp32 sum
        double s = 0.0;
        for (int k = 0; k < p.K; ++k) {
            const long j = j0 + k;
            if (j >= 0 && j < L) s = fma((double)kr[k], (double)x[j], s);
        }
        out = (float)s;
    } else {
        float s = 0.f;
        for (int k = 0; k < p.K; ++k) {
            const long j = j0 + k;
            if (j >= 0 && j < L) s = fmaf(kr[k], x[j], s);
        }
        out = s;
    }
    p.y[(long)b * p.y_sb + i] = out;
}

// x0[b][t][f] = scale * mel[b][f][t] + shift for t < T_b, the BatchNorm of the zero padding (shift) for T_b <= t < Tp_b
__global__ __launch_bounds__(256) void rm_prep_kernel(const RmPrepP p) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)(idx / 128), f = (int)(idx % 128);
    if (t >= p.Tp[b]) return;
    const float v = t < p.T[b] ? p.mel[(long)b * p.sb + (long)f * p.sm + (long)t * p.st] : 0.f;
    p.x[((long)b * p.Tal + t) * 128 + f] = fmaf(p.scale, v, p.shift);
}

// 8 consecutive floats at a 16-byte aligned byte offset through the store primitive of dsd_device.h
__device__ __forceinline__ void st8(const dsd_i32x4& r, int off, const float (&v)[RM_CO]) {
    st4_l2(f32x4{v[0], v[1], v[2], v[3]}, r, off, 0);
    st4_l2(f32x4{v[4], v[5], v[6], v[7]}, r, off + 16, 0);
}

// ---------------------------------------------------------------------------------------------
// One thread = one 2x2 quad of (frame, bin) positions x 8 output channels; blockIdx.y = the channel group, so every weight
// read is wave-uniform.  The K walk is tap-major, then channels in vectors of CIV (one 16-byte load per
// position when the channel counts allow); each weight vector serves 4 positions.  Positions outside [0, Tl) x [0, F) of
// the item are the conv's zero padding.  work: (b, first quad, Tl).
// ---------------------------------------------------------------------------------------------
template <int CIV>
__global__ __launch_bounds__(256) void rm_conv3_kernel(const RmConvP p) {
    const int* e = p.work + 3 * blockIdx.x;
    const int b = e[0], Tl = e[2], F = p.F, FQ = F >> 1;
    const int q = e[1] + threadIdx.x;
    if (q >= ((Tl + 1) >> 1) * FQ) return;
    const int t0 = 2 * (q / FQ), f0 = 2 * (q % FQ), co0 = blockIdx.y * RM_CO;
    const int cin = p.c0 + p.c1;
    float acc[4][RM_CO];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) acc[i][o] = 0.f;
    for (int s = 0; s < 2; ++s) {
        const int cs = s ? p.c1 : p.c0, cb = s ? p.c0 : 0;
        if (cs == 0) continue;
        const float* __restrict__ src = (s ? p.x1 : p.x0) + (long)b * p.Tal * F * cs;
#pragma unroll 1
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll 1
            for (int kf = 0; kf < 3; ++kf) {
                bool in[2][2];
                long off[2][2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int t = t0 + i + kt - 1, f = f0 + j + kf - 1;
                        in[i][j] = t >= 0 && t < Tl && f >= 0 && f < F;
                        off[i][j] = in[i][j] ? ((long)t * F + f) * cs : 0;
                    }
                const float* wt = p.w + ((long)(kt * 3 + kf) * cin + cb) * p.cout_pad + co0;
                // weights through vector loads (all lanes one address): as scalar loads, four vectors of 8 next to the kernel
                // arguments spill SGPRs
                asm volatile("" : "+v"(wt));
#pragma unroll 1
                for (int ci = 0; ci < cs; ci += CIV) {
                    float v[2][2][CIV];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if constexpr (CIV == 4) {
                                const f32x4 x4 = in[i][j] ? *(const f32x4*)(src + off[i][j] + ci) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                                for (int c = 0; c < 4; ++c) v[i][j][c] = x4[c];
                            } else {
                                v[i][j][0] = in[i][j] ? src[off[i][j] + ci] : 0.f;
                            }
                        }
#pragma unroll
                    for (int c = 0; c < CIV; ++c) {
                        const float* __restrict__ w = wt + (long)(ci + c) * p.cout_pad;
                        float wv[RM_CO];
#pragma unroll
                        for (int o = 0; o < RM_CO; ++o) wv[o] = w[o];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int o = 0; o < RM_CO; ++o)
                                    acc[2 * i + j][o] = fmaf(v[i][j][c], wv[o], acc[2 * i + j][o]);
                    }
                }
            }
    }
    // epilogue: folded BN shift (or the conv bias), ReLU, residual
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) {
            const float y = acc[i][o] + p.shift[co0 + o];
            acc[i][o] = p.relu ? fmaxf(y, 0.f) : y;
        }
    if (p.res_mode == 1) {              // identity: the block input, cout channels
        const float* __restrict__ r = p.r0 + (long)b * p.Tal * F * p.rc0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + (i >> 1), f = f0 + (i & 1);
            if (t >= Tl) continue;
#pragma unroll
            for (int o = 0; o < RM_CO; ++o)
                if (co0 + o < p.cout) acc[i][o] += r[((long)t * F + f) * p.rc0 + co0 + o];
        }
    } else if (p.res_mode == 2) {       // shortcut: Conv2d(cin, cout, 1) with bias over the block input (concat or not)
        float sc[4][RM_CO];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int o = 0; o < RM_CO; ++o) sc[i][o] = 0.f;
        for (int s = 0; s < 2; ++s) {
            const int cs = s ? p.rc1 : p.rc0, cb = s ? p.rc0 : 0;
            if (cs == 0) continue;
            const float* __restrict__ src = (s ? p.r1 : p.r0) + (long)b * p.Tal * F * cs;
#pragma unroll 1
            for (int ci = 0; ci < cs; ++ci) {
                const float* __restrict__ w = p.ws + (long)(cb + ci) * p.cout_pad + co0;
                float wv[RM_CO];
#pragma unroll
                for (int o = 0; o < RM_CO; ++o) wv[o] = w[o];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = min(t0 + (i >> 1), Tl - 1), f = f0 + (i & 1);
                    const float xv = src[((long)t * F + f) * cs + ci];
#pragma unroll
                    for (int o = 0; o < RM_CO; ++o) sc[i][o] = fmaf(xv, wv[o], sc[i][o]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int o = 0; o < RM_CO; ++o) acc[i][o] += sc[i][o] + p.bs[co0 + o];
    }
    const dsd_i32x4 ry = dsd_rsrc_words(p.y);
    const long ybase = (long)b * p.Tal * F;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + (i >> 1), f = f0 + (i & 1);
        if (t >= Tl) continue;
        const long pos = ybase + (long)t * F + f;
        if ((p.cout & 7) == 0) {
            st8(ry, (int)((pos * p.cout + co0) * 4), acc[i]);
        } else {
#pragma unroll
            for (int o = 0; o < RM_CO; ++o)
                if (co0 + o < p.cout) p.y[pos * p.cout + co0 + o] = acc[i][o];
        }
    }
    if (p.pool) {                        // AvgPool2d(2): ((x00 + x01) + x10) + x11, / 4, as torch's CPU kernel sums
        float pv[RM_CO];
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) pv[o] = (((acc[0][o] + acc[1][o]) + acc[2][o]) + acc[3][o]) / 4.f;
        const long pos = ((long)b * (p.Tal >> 1) + (t0 >> 1)) * (F >> 1) + (f0 >> 1);
        st8(dsd_rsrc_words(p.pool), (int)((pos * p.cout + co0) * 4), pv);
    }
}

// ---------------------------------------------------------------------------------------------
// ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1): one thread = input position (i, j) -> the output quad
// (2i + a, 2j + c), the four parity sub-convolutions.  Output row 2i reads input i with tap 1; row 2i + 1 reads input i with
// tap 2 and input i + 1 with tap 0 (zero past the item's Tin frames / the F bins).  w: [kt * 3 + kf][cin][cout_pad], BN folded.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_tconv_kernel(const RmConvP p) {
    const int* e = p.work + 3 * blockIdx.x;
    const int b = e[0], Tin = e[2], F = p.F;
    const int q = e[1] + threadIdx.x;
    if (q >= Tin * F) return;
    const int ti = q / F, fi = q % F, co0 = blockIdx.y * RM_CO, cin = p.c0;
    const float* __restrict__ src = p.x0 + (long)b * p.Tal * F * cin;
    const bool tn = ti + 1 < Tin, fn = fi + 1 < F;
    float acc[4][RM_CO];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) acc[i][o] = 0.f;
    for (int ci = 0; ci < cin; ++ci) {
        const float x00 = src[((long)ti * F + fi) * cin + ci];
        const float x01 = fn ? src[((long)ti * F + fi + 1) * cin + ci] : 0.f;
        const float x10 = tn ? src[((long)(ti + 1) * F + fi) * cin + ci] : 0.f;
        const float x11 = tn && fn ? src[((long)(ti + 1) * F + fi + 1) * cin + ci] : 0.f;
        const float* __restrict__ w = p.w + (long)ci * p.cout_pad + co0;
        const long tap = (long)cin * p.cout_pad;
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) {
            const float w00 = w[0 * tap + o], w01 = w[1 * tap + o], w02 = w[2 * tap + o];
            const float w10 = w[3 * tap + o], w11 = w[4 * tap + o], w12 = w[5 * tap + o];
            const float w20 = w[6 * tap + o], w21 = w[7 * tap + o], w22 = w[8 * tap + o];
            acc[0][o] = fmaf(x00, w11, acc[0][o]);
            acc[1][o] = fmaf(x01, w10, fmaf(x00, w12, acc[1][o]));
            acc[2][o] = fmaf(x10, w01, fmaf(x00, w21, acc[2][o]));
            acc[3][o] = fmaf(x11, w00, fmaf(x10, w02, fmaf(x01, w20, fmaf(x00, w22, acc[3][o]))));
        }
    }
    const int Fo = 2 * F;
    const dsd_i32x4 ry = dsd_rsrc_words(p.y);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v[RM_CO];
#pragma unroll
        for (int o = 0; o < RM_CO; ++o) v[o] = fmaxf(acc[i][o] + p.shift[co0 + o], 0.f);
        const long pos = ((long)b * p.Tal * 2 + 2 * ti + (i >> 1)) * Fo + 2 * fi + (i & 1);
        st8(ry, (int)((pos * p.cout + co0) * 4), v);
    }
}

// ---------------------------------------------------------------------------------------------
// y[row][n] = act(sum_k x[row][k] W[k][n] + bias[n]) for the rows (b, t < Tp_b); one thread = one row x 8 outputs,
// blockIdx.y = the output group (uniform weight reads).  work: (b, first frame, Tp_b).  act 1 = sigmoid.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_linear_kernel(const RmLinearP p) {
    const int* e = p.work + 3 * blockIdx.x;
    const int b = e[0], t = e[1] + threadIdx.x;
    if (t >= e[2]) return;
    const long row = (long)b * p.Tal + t;
    const int n0 = blockIdx.y * RM_CO;
    const float* __restrict__ x = p.x + row * p.K;
    float acc[RM_CO];
#pragma unroll
    for (int o = 0; o < RM_CO; ++o) acc[o] = 0.f;
    for (int k = 0; k < p.K; k += 4) {
        const f32x4 xv = *(const f32x4*)(x + k);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float* __restrict__ w = p.w + (long)(k + c) * p.N + n0;
#pragma unroll
            for (int o = 0; o < RM_CO; ++o) acc[o] = fmaf(xv[c], w[o], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < RM_CO; ++o) {
        const float v = acc[o] + p.bias[n0 + o];
        acc[o] = p.act ? 1.f / (1.f + expf(-v)) : v;
    }
    st8(dsd_rsrc_words(p.y), (int)((row * p.N + n0) * 4), acc);
}

// ---------------------------------------------------------------------------------------------
// One GRU direction of one item: blockIdx = (item, direction).  Thread r < 768 owns row r of W_hh (gate r / z / n of unit
// r % 256): columns [0, RM_KR) in registers, [RM_KR, RM_KR + RM_KL) in LDS, the rest read from L2 each step in the
// [k][768] layout (coalesced).  Per step: gh = W_hh h + b_hh through LDS, then unit j < 256 applies
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h      (torch.nn.GRU)
// The item runs over its own Tp_b frames; the reverse direction starts at Tp_b - 1.  gi: [b][t][1536] (forward | reverse
// gates with b_ih), y: [b][t][512] (forward | reverse h).
// ---------------------------------------------------------------------------------------------
constexpr int RM_H = 256, RM_G = 768, RM_KR = 112, RM_KL = 48, RM_KG = RM_H - RM_KR - RM_KL;
__global__ __launch_bounds__(768) void rm_gru_kernel(const RmGruP p) {
    __shared__ __attribute__((aligned(16))) float sW[RM_KL * RM_G];
    __shared__ __attribute__((aligned(16))) float sh[RM_H];
    __shared__ float sg[RM_G];
    const int b = blockIdx.x, d = blockIdx.y, r = threadIdx.x, Tp = p.Tp[b];
    const float* __restrict__ whh = p.whh + (long)d * RM_H * RM_G;      // [k][768]
    float wr[RM_KR];
#pragma unroll
    for (int k = 0; k < RM_KR; ++k) wr[k] = whh[(long)k * RM_G + r];
    for (int k = 0; k < RM_KL; ++k) sW[k * RM_G + r] = whh[(long)(RM_KR + k) * RM_G + r];
    const float* __restrict__ wg = whh + (long)(RM_KR + RM_KL) * RM_G + r;
    const float bh = p.bhh[d * RM_G + r];
    if (r < RM_H) sh[r] = 0.f;
    __syncthreads();
    for (int s = 0; s < Tp; ++s) {
        const int t = d ? Tp - 1 - s : s;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k = 0; k < RM_KR; k += 4) {
            const f32x4 hv = *(const f32x4*)(sh + k);
            a0 = fmaf(wr[k], hv[0], a0);
            a1 = fmaf(wr[k + 1], hv[1], a1);
            a2 = fmaf(wr[k + 2], hv[2], a2);
            a3 = fmaf(wr[k + 3], hv[3], a3);
        }
#pragma unroll 4
        for (int k = 0; k < RM_KL; k += 4) {
            const f32x4 hv = *(const f32x4*)(sh + RM_KR + k);
            a0 = fmaf(sW[k * RM_G + r], hv[0], a0);
            a1 = fmaf(sW[(k + 1) * RM_G + r], hv[1], a1);
            a2 = fmaf(sW[(k + 2) * RM_G + r], hv[2], a2);
            a3 = fmaf(sW[(k + 3) * RM_G + r], hv[3], a3);
        }
#pragma unroll 4
        for (int k = 0; k < RM_KG; k += 4) {
            const f32x4 hv = *(const f32x4*)(sh + RM_KR + RM_KL + k);
            a0 = fmaf(wg[(long)k * RM_G], hv[0], a0);
            a1 = fmaf(wg[(long)(k + 1) * RM_G], hv[1], a1);
            a2 = fmaf(wg[(long)(k + 2) * RM_G], hv[2], a2);
            a3 = fmaf(wg[(long)(k + 3) * RM_G], hv[3], a3);
        }
        sg[r] = ((a0 + a1) + (a2 + a3)) + bh;
        __syncthreads();
        if (r < RM_H) {
            const float* __restrict__ gi = p.gi + ((long)b * p.Tal + t) * (2 * RM_G) + d * RM_G;
            const float rg = 1.f / (1.f + expf(-(gi[r] + sg[r])));
            const float zg = 1.f / (1.f + expf(-(gi[RM_H + r] + sg[RM_H + r])));
            const float ng = tanhf(fmaf(rg, sg[2 * RM_H + r], gi[2 * RM_H + r]));
            const float hn = fmaf(zg, sh[r] - ng, ng);       // (1 - z) n + z h
            sh[r] = hn;
            p.y[((long)b * p.Tal + t) * (2 * RM_H) + d * RM_H + r] = hn;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// to_local_average_f0 (utils.py:8-23): one wave per frame (b, t < T_b).  argmax over the 360 classes (first index on ties),
// the weighted mean of 20 i + CONST over [c - 4, c + 5) clipped to [0, 360), f0 = 10 * 2^(cents / 1200), 0 where max < thred.
// Optionally copies the frame's 360 values to hidden_out.  With p.center the window sits around that class instead of the
// argmax (to_local_average_f0(hidden, center=...), utils.py:11-14); the threshold still reads the frame's maximum.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_decode_kernel(const RmDecodeP p) {
    const int lane = threadIdx.x & 63;
    const long fr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = (int)(fr / p.Tmax), t = (int)(fr % p.Tmax);
    if (b >= p.B || t >= p.T[b]) return;
    const float* __restrict__ hv = p.hidden + (long)b * p.h_sb + (long)t * p.h_st;
    float best = -INFINITY;
    int bi = 360;
    for (int i = lane; i < 360; i += 64) {
        const float v = hv[i];
        if (v > best || bi == 360) {
            best = v;
            bi = i;
        }
        if (p.out_hidden) p.out_hidden[(long)b * p.o_sb + (long)t * p.o_st + i] = v;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane != 0 || !p.f0) return;
    if (p.center) bi = min(max(p.center[(long)b * p.c_sb + t], 0), 359);     // the threshold still reads the frame's maximum
    const int lo = max(bi - 4, 0), hi = min(bi + 5, 360);
    float ps = 0.f, ws = 0.f;
    for (int i = lo; i < hi; ++i) {
        ps = fmaf(hv[i], 20.f * (float)i + 1997.3794084376191f, ps);
        ws += hv[i];
    }
    const float cents = ps / (ws + (ws == 0.f ? 1.f : 0.f));
    const float f0 = 10.f * exp2f(cents / 1200.f);
    p.f0[(long)b * p.f_sb + t] = best < p.thred ? 0.f : f0;
}

// ---------------------------------------------------------------------------------------------
// to_viterbi_f0 (utils.py:26-43) = librosa.sequence.viterbi (0.9.2) over 360 states, in double from the fp32 hidden:
//   log_prob[t][j] = log(hidden[t][j] / sum_i hidden[t][i] + eps), eps = the float32 tiny (what a zero probability and a
//   jump of 30 classes or more cost: log(eps) = -87.34)
//   value[0] = log_prob[0] + log(1 / 360 + eps);   value[t][j] = log_prob[t][j] + max_k (value[t - 1][k] + log_trans[k][j]),
//   ptr[t][j] = the first k at that maximum;   state[T - 1] = argmax value[T - 1], state[t] = ptr[t + 1][state[t + 1]]
// rm_logprob_kernel: one wave per frame (b, t < T_b) writes the frame's log_prob row.
// ---------------------------------------------------------------------------------------------
constexpr int VT_S = 360, VT_THREADS = 384, VT_WAVES = VT_THREADS / 64, VT_PAD = VT_THREADS + RM_VT_W - 1;
constexpr int VT_ROWS = 32, VT_ROW_DW = VT_S / 2, VT_PRE = VT_ROWS * VT_ROW_DW / VT_THREADS;
static_assert(VT_PRE * VT_THREADS == VT_ROWS * VT_ROW_DW, "a chunk of back-pointer rows is a whole number of dwords per thread");

__global__ __launch_bounds__(256) void rm_logprob_kernel(const RmViterbiP p) {
    const int lane = threadIdx.x & 63;
    const long fr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = (int)(fr / p.Tmax), t = (int)(fr % p.Tmax);
    if (b >= p.B || t >= p.T[b]) return;
    const float* __restrict__ hv = p.hidden + (long)b * p.h_sb + (long)t * p.h_st;
    double s = 0.0;
    for (int i = lane; i < VT_S; i += 64) s += (double)hv[i];
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    double* __restrict__ lp = p.lp + ((long)b * p.Tmax + t) * VT_S;
    for (int i = lane; i < VT_S; i += 64) lp[i] = log((double)hv[i] / s + p.eps);
}

// value[t] of thread j's state into the step's LDS buffer, and the wave's first-index argmax of it; ends in the step's barrier
__device__ __forceinline__ void vt_publish(double v, int j, double* sv, double* wv, int* wk) {
    if (j < VT_S) sv[j + RM_VT_BAND] = v;
    double m = v;
    int k = j;
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(m, off);
        const int ok = __shfl_xor(k, off);
        if (ov > m || (ov == m && ok < k)) {
            m = ov;
            k = ok;
        }
    }
    if ((j & 63) == 0) {
        wv[j >> 6] = m;
        wk[j >> 6] = k;
    }
    __syncthreads();
}
// the workgroup's first-index argmax from the waves' (ascending classes: a strict > keeps the first index)
__device__ __forceinline__ void vt_argmax(const double* wv, const int* wk, double& gv, int& gk) {
    gv = wv[0];
    gk = wk[0];
#pragma unroll
    for (int q = 1; q < VT_WAVES; ++q)
        if (wv[q] > gv) {
            gv = wv[q];
            gk = wk[q];
        }
    gk = min(gk, VT_S - 1);         // NaN input (a frame that sums to zero) compares false everywhere: keep every index a state
}

// ---------------------------------------------------------------------------------------------
// rm_viterbi_kernel: one workgroup per item, thread j owns state j, the item's own T_b steps.  value[t - 1] sits in LDS
// (double-buffered, -inf on 29 classes either side), the 59 transition terms of column j in registers.  Outside the band
// every candidate is value[t - 1][k] + log(eps), so the only one that can win is the workgroup's first-index argmax k* of
// value[t - 1], and only where |k* - j| >= 30; first index on ties throughout.  One barrier per step.
// The backtrack follows in the same workgroup: the back-pointer rows to visit are known (T_b - 1 .. 1), only the column is
// not, so a chunk of 32 rows is fetched by all threads into registers while thread 0 walks the previous chunk in LDS.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT_THREADS) void rm_viterbi_kernel(const RmViterbiP p) {
    __shared__ double sv[2][VT_PAD];
    __shared__ double wv[2][VT_WAVES];
    __shared__ int wk[2][VT_WAVES];
    __shared__ unsigned int srow[VT_ROWS * VT_ROW_DW];
    __shared__ int spath[VT_ROWS];
    const int b = blockIdx.x, j = threadIdx.x, T = p.T[b];
    const bool live = j < VT_S;
    double w[RM_VT_W];
#pragma unroll
    for (int d = 0; d < RM_VT_W; ++d) w[d] = live ? p.tab[d * VT_S + j] : 0.0;
    for (int i = j; i < 2 * VT_PAD; i += VT_THREADS) (&sv[0][0])[i] = -INFINITY;
    __syncthreads();
    const double* __restrict__ lp = p.lp + (long)b * p.Tmax * VT_S;
    unsigned short* ptr = p.ptr + (long)b * p.Tmax * VT_S;
    int cur = 0;
    vt_publish(live ? lp[j] + p.log_p_init : -INFINITY, j, sv[0], wv[0], wk[0]);
    for (int t = 1; t < T; ++t) {
        const double lpt = live ? lp[(long)t * VT_S + j] : 0.0;
        const double* pv = sv[cur] + j;         // pv[d] = value[t - 1][j + d - 29]
        double best = -INFINITY;
        int bd = RM_VT_BAND;
#pragma unroll
        for (int d = 0; d < RM_VT_W; ++d) {
            const double c = pv[d] + w[d];
            if (c > best) {
                best = c;
                bd = d;
            }
        }
        int bk = j + bd - RM_VT_BAND;
        double gv;
        int gk;
        vt_argmax(wv[cur], wk[cur], gv, gk);
        if (abs(gk - j) > RM_VT_BAND) {
            const double c = gv + p.log_eps;
            if (c > best || (c == best && gk < bk)) {
                best = c;
                bk = gk;
            }
        }
        if (live) ptr[(long)t * VT_S + j] = (unsigned short)bk;
        cur ^= 1;
        vt_publish(live ? lpt + best : -INFINITY, j, sv[cur], wv[cur], wk[cur]);
    }
    double gv;
    int state;
    vt_argmax(wv[cur], wk[cur], gv, state);
    int* __restrict__ center = p.center + (long)b * p.Tmax;
    int* __restrict__ path = p.path_out ? p.path_out + (long)b * p.p_sb : nullptr;
    if (j == 0) {
        center[T - 1] = state;
        if (path) path[T - 1] = state;
    }
    // rows hi .. lo (descending) give state[hi - 1] .. state[lo - 1]; the stores above are this workgroup's own, behind a barrier
    unsigned int pre[VT_PRE];
    auto fetch = [&](int hi) {
        const int lo = max(hi - VT_ROWS + 1, 1), n = (hi - lo + 1) * VT_ROW_DW;
        const unsigned int* src = reinterpret_cast<const unsigned int*>(ptr + (long)lo * VT_S);
#pragma unroll
        for (int q = 0; q < VT_PRE; ++q) {
            const int i = j + q * VT_THREADS;
            pre[q] = i < n ? src[i] : 0u;
        }
    };
    if (T > 1) fetch(T - 1);
    for (int hi = T - 1; hi >= 1; hi -= VT_ROWS) {
        const int lo = max(hi - VT_ROWS + 1, 1), n = hi - lo + 1;
#pragma unroll
        for (int q = 0; q < VT_PRE; ++q) srow[j + q * VT_THREADS] = pre[q];
        __syncthreads();
        if (hi - VT_ROWS >= 1) fetch(hi - VT_ROWS);
        if (j == 0) {
            const unsigned short* rows = reinterpret_cast<const unsigned short*>(srow);
            for (int r = n - 1; r >= 0; --r) {
                state = min((int)rows[r * VT_S + state], VT_S - 1);
                spath[r] = state;
            }
        }
        __syncthreads();
        if (j < n) {
            center[lo - 1 + j] = spath[j];
            if (path) path[lo - 1 + j] = spath[j];
        }
    }
}

hipError_t launch_rm_resample(const RmResampleP& p, int B, long max_blocks, int nw, hipStream_t st) {
    hipLaunchKernelGGL(rm_resample_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)nw, (unsigned)B), dim3(256), 0,
                       st, p);
    return hipGetLastError();
}
hipError_t launch_rm_prep(const RmPrepP& p, int B, int Tal, hipStream_t st) {
    hipLaunchKernelGGL(rm_prep_kernel, dim3((unsigned)((Tal * 128 + 255) / 256), (unsigned)B), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_conv3(const RmConvP& p, int n_entries, hipStream_t st) {
    const dim3 grid((unsigned)n_entries, (unsigned)(p.cout_pad / RM_CO));
    if (p.c0 % 4 == 0 && p.c1 % 4 == 0) hipLaunchKernelGGL(rm_conv3_kernel<4>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(rm_conv3_kernel<1>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_tconv(const RmConvP& p, int n_entries, hipStream_t st) {
    hipLaunchKernelGGL(rm_tconv_kernel, dim3((unsigned)n_entries, (unsigned)(p.cout_pad / RM_CO)), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_linear(const RmLinearP& p, int n_entries, hipStream_t st) {
    hipLaunchKernelGGL(rm_linear_kernel, dim3((unsigned)n_entries, (unsigned)(p.N / RM_CO)), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_gru(const RmGruP& p, int B, hipStream_t st) {
    hipLaunchKernelGGL(rm_gru_kernel, dim3((unsigned)B, 2), dim3(RM_G), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_decode(const RmDecodeP& p, hipStream_t st) {
    const long frames = (long)p.B * p.Tmax;
    hipLaunchKernelGGL(rm_decode_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_rm_viterbi(const RmViterbiP& p, hipStream_t st) {
    const long frames = (long)p.B * p.Tmax;
    hipLaunchKernelGGL(rm_logprob_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(rm_viterbi_kernel, dim3((unsigned)p.B), dim3(VT_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace dsd
