// The score algebra of the variance front end (dsd_word_dur, dsd_group_midi, dsd_rhythm_align): what stands between a
// score's notes and phones and the variance twin's stage inputs, and between its predicted and its final durations.
//   word_dur_kernel      word durations from ph2word or from the note slurs, aligned to a frame count
//                        (inference/ds_variance.py:185-206)
//   group_midi_kernel    the rounded per-phone or per-word mean of the frame MIDI curve (inference/ds_variance.py:219-241)
//   rhythm_align_kernel  RhythmRegulator.forward (modules/fastspeech/tts_modules.py:250-275)
// One workgroup of 256 lanes per item; a row of at most 2048 entries sits in LDS.  The integer results do not depend on the
// order of any sum (int64 adds are exact); every fp32 sum runs in ONE lane in the order the interface states, and each
// division, product and addition is rounded to fp32 on its own: contraction is off for the whole file (acoustic_kernels.hip
// says why the pragma and not __fadd_rn / __fmul_rn: those do not stop the compiler from fusing what surrounds them).
#include "dsd_internal.h"
#include "dsd_device.h"
#include "words_params.h"

#pragma clang fp contract(off)

namespace dsd {

static_assert(kWordsMax == kRegulateMaxTokens, "words_params.h restates dsd_internal.h");
static_assert(kWordsMax <= 8 * 256, "block_prefix_capped takes 8 values per lane");

// ---------------------------------------------------------------------------------------------
// index[i] = ph2word[i], or with slurs the inclusive count of the non-slur notes up to note i (cumsum(~is_slur));
// word_dur[w - 1] = the int64 sum of dur[i] over index[i] == w (LDS atomics: exact in any order; an index outside [1, W]
// adds nothing).  With a total: c[w] = min(word_dur[0] + .. + word_dur[w], total), the durations become c[w] - c[w - 1], and
// the last word with a non-zero duration takes total - c[W - 1] on top.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void word_dur_kernel(const WordDurP p) {
    __shared__ unsigned long long wd[kWordsMax];
    __shared__ int cum[kWordsMax];
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const long b = p.b0 + (long)blockIdx.x;
    const int N = p.N, W = p.W;
    const int64_t* dur = p.dur + b * N;
    for (int w = tid; w < W; w += 256) wd[w] = 0ull;
    if (p.slur) {
        const uint8_t* slur = p.slur + b * N;
        block_prefix_capped(cum, part, N, N, [&](int i) { return slur[i] ? 0ll : 1ll; });
    } else {
        __syncthreads();
    }
    const int64_t* index = p.slur ? nullptr : p.index + b * N;
    for (int i = tid; i < N; i += 256) {
        const long long idx = index ? (long long)index[i] : (long long)cum[i];
        if (p.index_out) p.index_out[b * N + i] = idx;
        if (idx >= 1 && idx <= W) atomicAdd(&wd[idx - 1], (unsigned long long)dur[i]);
    }
    __syncthreads();
    int64_t* out = p.word_dur + b * W;
    if (!p.has_totals) {
        for (int w = tid; w < W; w += 256) out[w] = (int64_t)wd[w];
        return;
    }
    const int total = p.total[blockIdx.x];
    int last = -1;                                          // this lane's last word with a non-zero duration
    for (int w = tid; w < W; w += 256)
        if ((long long)wd[w] > 0) last = w;
    block_prefix_capped(cum, part, W, total, [&](int w) {
        const long long v = (long long)wd[w];
        return v > 0 ? min(v, (long long)total) : 0ll;
    });
    part[tid] = last;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] = max(part[tid], part[tid + s]);
        __syncthreads();
    }
    last = part[0];
    const int rest = total - cum[W - 1];
    for (int w = tid; w < W; w += 256) out[w] = (int64_t)(cum[w] - (w ? cum[w - 1] : 0) + (w == last ? rest : 0));
}

const char* launch_word_dur(const WordDurP& p, int items, void* stream) {
    word_dur_kernel<<<dim3(items), 256, 0, (hipStream_t)stream>>>(p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------
// Frames belong to notes and to groups as length_regulate_kernel assigns them: note j owns [cn[j - 1], cn[j]), group g owns
// [cg[g - 1], cg[g]), both sums capped at T.  One lane per group (a group's sum is one dependent chain): it finds the note of
// its first frame by binary search and walks its frames in order, adding note_midi[j] / (float)group_dur[g] once per frame - a
// quotient is computed once per note and added once per frame, never multiplied by the frame count.  A frame at or past the
// notes' total has MIDI 0 and adds +0.0f, which changes no sum: the walk ends there.  r[g] = rintf(sum) (half to even).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_midi_kernel(const GroupMidiP p) {
    __shared__ int cn[kWordsMax];
    __shared__ int cg[kWordsMax];
    __shared__ float r[kWordsMax];
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int Nn = p.Nn, G = p.G, T = p.T;
    const int64_t* nd = p.note_dur + b * Nn;
    const int64_t* gd = p.group_dur + b * G;
    const float* midi = p.note_midi + b * Nn;
    auto capped = [T](long long v) { return v > 0 ? min(v, (long long)T) : 0ll; };
    block_prefix_capped(cn, part, Nn, T, [&](int i) { return capped(nd[i]); });
    block_prefix_capped(cg, part, G, T, [&](int i) { return capped(gd[i]); });
    for (int g = tid; g < G; g += 256) {
        const int end = cg[g];
        int f = g ? cg[g - 1] : 0;
        float sum = 0.0f;
        if (f < end) {
            const float n = (float)gd[g];
            int j = first_above(cn, Nn, f);
            while (f < end && j < Nn) {
                const int stop = min(end, cn[j]);
                const float q = midi[j] / n;
                for (; f < stop; ++f) sum = sum + q;
                ++j;
            }
        }
        r[g] = rintf(sum);
    }
    __syncthreads();
    if (p.ph2word) {
        const int64_t* idx = p.ph2word + b * p.L;
        int64_t* out = p.midi + b * p.L;
        for (int i = tid; i < p.L; i += 256) {
            const long long w = idx[i];
            out[i] = (w >= 1 && w <= G) ? (int64_t)r[w - 1] : 0;
        }
    } else {
        int64_t* out = p.midi + b * G;
        for (int g = tid; g < G; g += 256) out[g] = (int64_t)r[g];
    }
}

const char* launch_group_midi(const GroupMidiP& p, int items, void* stream) {
    group_midi_kernel<<<dim3(items), 256, 0, (hipStream_t)stream>>>(p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------
// d[i] = pred[i] * (ph2word[i] > 0); s[w] = 0.0f + d[i0] + d[i1] + .. over ph2word[i] == w in index order, by ONE lane per
// word that scans the row in LDS (every lane of a wave reads the same address: a broadcast), so ph2word may stand in any
// order; alpha[w] = (float)word_dur[w - 1] / max(s[w], 1e-5f); out[i] = rintf(d[i] * alpha[ph2word[i]]).  An index outside
// [1, W] is kept as 0: it adds nothing and its duration is 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rhythm_align_kernel(const RhythmP p) {
    __shared__ int idx[kWordsMax];
    __shared__ float d[kWordsMax];
    __shared__ float alpha[kWordsMax];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int L = p.L, W = p.W;
    const int64_t* ph2word = p.ph2word + b * L;
    const float* pred = p.pred + b * L;
    const int64_t* wdur = p.word_dur + b * W;
    for (int i = tid; i < L; i += 256) {
        const long long w = ph2word[i];
        idx[i] = (w >= 1 && w <= W) ? (int)w : 0;
        d[i] = pred[i] * (w > 0 ? 1.0f : 0.0f);
    }
    __syncthreads();
    for (int w = tid; w < W; w += 256) {
        float s = 0.0f;
        for (int i = 0; i < L; ++i)
            if (idx[i] == w + 1) s = s + d[i];
        alpha[w] = (float)wdur[w] / (s < 1e-5f ? 1e-5f : s);
    }
    __syncthreads();
    int64_t* out = p.out + b * L;
    for (int i = tid; i < L; i += 256) out[i] = idx[i] ? (int64_t)rintf(d[i] * alpha[idx[i] - 1]) : 0;
}

const char* launch_rhythm_align(const RhythmP& p, int items, void* stream) {
    rhythm_align_kernel<<<dim3(items), 256, 0, (hipStream_t)stream>>>(p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace dsd
