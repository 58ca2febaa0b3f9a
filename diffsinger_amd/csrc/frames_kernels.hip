// Duration-to-frame stages of the deployment twins (dsd_length_regulate, dsd_frame_curve): what an editor's staged calls
// do between the token-level encoders and the frame-level condition.  Two small launches; the smoothing sums in fp64.
//   length_regulate_kernel   LengthRegulator.forward (deployment/modules/fastspeech2.py:31-40): durations -> mel2x
//   frame_curve_kernel       frame MIDI gather + the replicate-padded sinusoidal smoothing + the retake blend
//                            (deployment/modules/toplevel.py:179-194, 251-258)
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

// ---------------------------------------------------------------------------------------------
// mel2x[b][p] = i + 1 with cum[i - 1] <= p < cum[i], 0 at or past the item's total (the reference's masked sum over a
// [B, L, T] mask adds nothing there).  One workgroup per item: the inclusive prefix sum of the L <= 2048 durations sits in
// LDS, then every frame looks its token up by binary search (the first i with cum[i] > p; a zero duration repeats its
// predecessor's sum and is never the first).  Sums saturate at T: only p < T is ever asked, so the answer is the same and
// no sum overflows; a negative duration counts as 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void length_regulate_kernel(const long long* __restrict__ dur, int L, int T,
                                                              long long* __restrict__ mel2x) {
    __shared__ int cum[kRegulateMaxTokens];
    __shared__ int part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long* d = dur + (long)b * L;
    block_prefix_capped(cum, part, L, T, [&](int i) {
        const long long v = d[i];
        return v > 0 ? min(v, (long long)T) : 0ll;
    });
    long long* out = mel2x + (long)b * T;
    for (int p = tid; p < T; p += 256) {
        const int a = first_above(cum, L, p);
        out[p] = a < L ? a + 1 : 0;
    }
}

hipError_t launch_length_regulate(const long long* dur, int B, int L, int T, long long* mel2x, hipStream_t st) {
    length_regulate_kernel<<<dim3(B), 256, 0, st>>>(dur, L, T, mel2x);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// x[j] = mel2note[b][j] in [1, N] ? note_midi[b][mel2note[b][j] - 1] : 0   (gather from the source padded by one in front)
// base[t] = sum_k w[k] * x[clamp(t - left + k, 0, len_b - 1)],  left = (K - 1) / 2   (Conv1d, padding 'same', replicate)
// blend[t] = base[t] * retake[t] + pitch[t] * !retake[t];  delta[t] = (pitch[t] - base[t]) * !retake[t]
// One workgroup per 256 frames of an item: the 256 + K - 1 gathered values it needs are staged in LDS once, clamped to the
// item's own frames, so nothing at or past len_b is read.  Frames at or past len_b are written as 0.  The taps are summed
// in fp64 and rounded once, so the result is within one fp32 rounding of the exact sum whatever order torch's convolution takes.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void frame_curve_kernel(const FrameCurveP p) {
    __shared__ float x[256 + kCurveMaxTaps - 1];
    const int b = blockIdx.y, t0 = blockIdx.x * 256, tid = threadIdx.x;
    const int len = p.len[b];
    const long row = (long)(p.b0 + b) * p.T;
    const int left = (p.K - 1) >> 1;
    if (t0 < len) {
        const long long* idx = p.mel2note + row;
        const float* src = p.note_midi + (long)(p.b0 + b) * p.N;
        for (int j = tid; j < 256 + p.K - 1; j += 256) {
            const int t = min(max(t0 - left + j, 0), len - 1);
            const long long i = idx[t];
            x[j] = (i >= 1 && i <= p.N) ? src[i - 1] : 0.f;
        }
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t >= p.T) return;
    float base = 0.f, blend = 0.f, delta = 0.f;
    if (t < len) {
        double acc = 0.0;                                  // exact products, one rounding at the end: K <= 255 taps a frame
        for (int k = 0; k < p.K; ++k) acc += (double)p.w[k] * (double)x[tid + k];
        base = (float)acc;
        const float r = p.retake[row + t] ? 1.f : 0.f, nr = 1.f - r, pit = p.pitch[row + t];
        blend = base * r + pit * nr;
        delta = (pit - base) * nr;
    }
    p.base[row + t] = base;
    p.blend[row + t] = blend;
    p.delta[row + t] = delta;
}

hipError_t launch_frame_curve(const FrameCurveP& p, int items, hipStream_t st) {
    frame_curve_kernel<<<dim3((p.T + 255) / 256, items), 256, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace dsd
