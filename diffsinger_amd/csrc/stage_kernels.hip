// The variance twin's stage kernels (dsd_variance_*, variance_api.hip): the index arithmetic and per-frame scalars that
// deployment/modules/fastspeech2.py:145-184 and toplevel.py:224-302 write as torch.gather / F.pad / isin / mask products
// around the encoders, and the mean over the repeat bins behind the samplers.  All are latency-bound on tiny grids (a
// few hundred tokens, a few thousand frames): one launch each, lanes along the tokens or frames, no LDS but the wave
// reduction's registers.  What they write feeds assemble_kernel (encoder_kernels.hip) with the operands, and in the order,
// of diffsinger_amd/deploy.py, so the assembled conditions are bit-identical to the Python twin's.
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

// ---------------------------------------------------------------------------------------------
// forward_linguistic_encoder_word (fastspeech2.py:145-161) after the length regulator, per phoneme l of item b:
//   onset[l]   = ph2word[l] > ph2word[l - 1]  (0 in front: F.pad(ph2word, [1, -1]))
//   dur_f[l]   = float(pad(word_dur, [1, 0])[ph2word[l]])         a word index outside [1, W] reads 0
//   lang[l]    = languages[l] * mask[tokens[l]]                   _masked_languages: isin(tokens, cross_lingual_token_idx)
//   x_masks[l] = tokens[l] == 0
// The phoneme form (:163-176) has no ph2word: dur_f = float(ph_dur), onset is not read.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_encode_kernel(const StageEncodeP p) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= p.L) return;
    const long i = (long)b * p.L + l;
    const long long tok = p.tokens[i];
    long long onset = 0, dur = 0;
    if (p.ph2word) {
        const long long w = p.ph2word[i], before = l > 0 ? p.ph2word[i - 1] : 0;
        onset = w > before ? 1 : 0;
        dur = (w >= 1 && w <= p.W) ? p.word_dur[(long)b * p.W + (w - 1)] : 0;
    } else {
        dur = p.ph_dur[i];
    }
    long long lang = 0;
    if (p.languages) {
        const bool cross = tok >= 0 && tok < p.vocab && p.mask[tok] != 0.f;
        lang = cross ? p.languages[i] : 0;
    }
    p.onset[i] = onset;
    p.dur_f[i] = (float)dur;
    p.lang[i] = lang;
    p.x_masks[i] = tok == 0 ? 1 : 0;
}

hipError_t launch_stage_encode(const StageEncodeP& p, int B, hipStream_t st) {
    stage_encode_kernel<<<dim3((p.L + 255) / 256, B), 256, 0, st>>>(p);
    return hipGetLastError();
}

// iota[b][l] = l (the gather of a [B, L, H] tensor at its own rows) and the speaker gather's index: l or 0
__global__ __launch_bounds__(256) void stage_iota_kernel(long long* __restrict__ iota, long long* __restrict__ spk_idx, int spk_iota,
                                                         int L) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= L) return;
    const long i = (long)b * L + l;
    iota[i] = l;
    if (spk_idx) spk_idx[i] = spk_iota ? l : 0;
}

hipError_t launch_stage_iota(long long* iota, long long* spk_idx, int spk_iota, int B, int L, hipStream_t st) {
    stage_iota_kernel<<<dim3((L + 255) / 256, B), 256, 0, st>>>(iota, spk_idx, spk_iota, L);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// MelodyEncoder.forward (variance_encoder.py:130-146), per note: keep = !rest,
//   midi_s = note_midi * keep * sqrt(h)   two fp32 products, in this order
//   keep_s = keep * sqrt(h);  dur_f = float(note_dur);  glide = note_glide or 0;  pad = note_midi < 0
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_notes_kernel(const StageNoteP p) {
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= p.N) return;
    const long i = (long)b * p.N + n;
    const float midi = p.note_midi[i], keep = p.note_rest[i] ? 0.f : 1.f;
    const float mk = midi * keep;
    p.midi_s[i] = mk * p.scale;
    p.keep_s[i] = keep * p.scale;
    p.dur_f[i] = (float)p.note_dur[i];
    p.glide[i] = p.note_glide ? p.note_glide[i] : 0;
    p.pad[i] = midi < 0.f ? 1 : 0;
}

hipError_t launch_stage_notes(const StageNoteP& p, int B, hipStream_t st) {
    stage_notes_kernel<<<dim3((p.N + 255) / 256, B), 256, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Per frame.  The pitch form (toplevel.py:239-249): e = expr * retake (expr absent: retake), and 1 - e.
// The variance form (:279-287): keep_v = !retake[b][t][v], kept_v = curve_v * keep_v.
// Either: the speaker gather's index, t for a [B, T, H] embedding and 0 for a [B, 1, H] one.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_frames_kernel(const StageFrameP p) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= p.T) return;
    const long i = (long)b * p.T + t;
    if (p.V == 0) {
        const float r = p.retake[i] ? 1.f : 0.f;
        const float e = p.expr ? p.expr[i] * r : r;
        p.e[i] = e;
        p.one_minus_e[i] = 1.0f - e;
    } else {
        for (int v = 0; v < p.V; ++v) {
            const float keep = p.retake[i * p.V + v] ? 0.f : 1.f;
            p.keep[v][i] = keep;
            p.kept[v][i] = p.curves[v][i] * keep;
        }
    }
    if (p.spk_idx) p.spk_idx[i] = p.spk_iota ? t : 0;
}

hipError_t launch_stage_frames(const StageFrameP& p, int B, hipStream_t st) {
    stage_frames_kernel<<<dim3((p.T + 255) / 256, B), 256, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// out_f[b][t] = clamp(mean_m sample[b][f][t][m]) (+ base[b][t]): the repeat bins' mean (deployment/modules/diffusion.py:
// 185-190, 217-222), clamp_spec, and the pitch form's base.  One wave per (b, f, t) row, lanes along the M bins: lane l adds
// m = l, l + 64, ... in that order, then the 64 partial sums fold by halving strides 32, 16, 8, 4, 2, 1 (lane l takes lane
// l ^ stride), so every lane ends with the same sum; lane 0 divides by M and writes.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_post_kernel(const StagePostP p, long rows) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                           // whole waves leave together: the shuffles below see full waves
    const float* x = p.sample + row * p.M;
    float acc = 0.f;
    for (int m = lane; m < p.M; m += 64) acc += x[m];
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if (lane != 0) return;
    const long ft = (long)p.F * p.T;
    const long b = row / ft;
    const int f = (int)((row - b * ft) / p.T), t = (int)(row - b * ft - (long)f * p.T);
    float v = acc / (float)p.M;
    if (p.clamp[f]) v = v < p.lo[f] ? p.lo[f] : (v > p.hi[f] ? p.hi[f] : v);       // torch.clamp: a NaN stays one
    const long o = b * p.T + t;
    if (p.base) v += p.base[o];
    p.out[f][o] = v;
}

hipError_t launch_stage_post(const StagePostP& p, int B, hipStream_t st) {
    const long rows = (long)B * p.F * p.T;
    stage_post_kernel<<<dim3((unsigned)((rows + 3) / 4)), 256, 0, st>>>(p, rows);
    return hipGetLastError();
}

}  // namespace dsd
