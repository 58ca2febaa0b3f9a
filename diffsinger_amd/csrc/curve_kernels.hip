// The segment front end's curves (dsd_curve_resample): resample_align_curve (utils/infer_utils.py:41-53) for up to 32
// curves of a segment or a ragged group in one launch, with what the inference front ends do to the result folded in.
//   curve_resample_kernel   np.interp over src_step * arange(n) at arange(0, (n - 1) * src_step, dst_step), cut / hold-last to
//                           `length`, zeros up to pad_to; then nothing, the clip (velocity, ds_acoustic.py:169-176), the
//                           gender -> key-shift map (ds_acoustic.py:154-159), or - for a PITCH curve - the raw f0 and uv
//   curve_pitch_kernel      interp_f0 + hz_to_midi (utils/pitch_utils.py:13-20, ds_variance.py:244-249) in place over that f0
// The resampling must equal numpy's double arithmetic bit for bit - every product and sum rounded on its own - so nothing
// here may be contracted into an fma: contraction is off for the whole file.
#include "../../include/dsdenoise.h"
#include "dsd_internal.h"
#include "dsd_device.h"
#include "curve_params.h"

#pragma clang fp contract(off)

namespace dsd {

// ---------------------------------------------------------------------------------------------
// One workgroup per kCurveChunk frames of one curve (blockIdx.y).  Frame t < length takes sample k = min(t, valid - 1):
// x = k * dst_step; j = the largest index with src_step * j <= x, from the quotient and a fix-up against the two products
// numpy's own table holds (xp[j] = src_step * j), so that j is numpy's binary-search answer whatever the quotient rounds to.
// Reads points[j], points[j + 1] with j + 1 <= n_points - 1 only; writes out[0 .. pad_to) and uv[0 .. pad_to).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCurveChunk) void curve_resample_kernel(const CurveBatch b) {
    const CurveD& c = b.c[blockIdx.y];
    const int t = blockIdx.x * kCurveChunk + threadIdx.x;
    if (t >= c.pad_to) return;
    if (t >= c.length) {
        c.out[t] = 0.f;
        if (c.uv) c.uv[t] = 0;
        return;
    }
    const int k = min(t, c.valid - 1);
    const double x = (double)k * c.dst_step;
    const int last = c.n_points - 1;
    int j = (int)fmin(x / c.src_step, (double)last);
    while (j > 0 && c.src_step * (double)j > x) --j;
    while (j < last && c.src_step * (double)(j + 1) <= x) ++j;
    float v;
    if (j >= last) {
        v = c.points[last];
    } else {
        const double xj = c.src_step * (double)j;
        const double pj = (double)c.points[j];
        if (xj == x) {
            v = (float)pj;
        } else {
            const double slope = ((double)c.points[j + 1] - pj) / (c.src_step * (double)(j + 1) - xj);
            v = (float)(slope * (x - xj) + pj);
        }
    }
    if (c.op == DSD_CURVE_CLIP) {
        v = fminf(fmaxf(v, c.lo), c.hi);
    } else if (c.op == DSD_CURVE_GENDER) {
        v = (float)((double)v * (v >= 0.f ? (double)c.hi : fabs((double)c.lo)));
        v = fminf(fmaxf(v, c.lo), c.hi);
    } else if (c.op == DSD_CURVE_PITCH && c.uv) {
        c.uv[t] = v == 0.f;
    }
    c.out[t] = v;
}

// ---------------------------------------------------------------------------------------------
// One workgroup per PITCH curve walks its frames in chunks of kCurveChunk, in place over the f0 the first launch left in
// out.  A voiced frame is finished at once.  An unvoiced frame needs the nearest voiced frame on either side: inside the
// chunk the four waves' ballots give both; the one before the chunk is the carry (index, log2 f0) of the walk; a run of
// unvoiced frames that reaches the end of the chunk stays pending (still 0 in out) until a later chunk brings its first
// voiced frame - or the curve ends, and the run takes the carry, or -inf when nothing was voiced at all.  Every frame is
// read once, by the thread of its own chunk, before anything of this launch writes it, and written once.
// log2 f0 is rounded to fp32 as the host path stores it (np.log2 of an fp32 array, np.interp's double stored into it),
// the filled f0 = 2 ** logf likewise, and the MIDI value at the end; everything between is double.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float pitch_finish(float logf, double log2_440) {
    const float f = (float)exp2((double)logf);
    return (float)(12.0 * (log2((double)f) - log2_440) + 69.0);
}
__device__ __forceinline__ float pitch_between(int t, int pi, float pl, int ni, float nl) {
    const double slope = ((double)nl - (double)pl) / ((double)ni - (double)pi);      // np.interp over the voiced indices
    return (float)(slope * ((double)t - (double)pi) + (double)pl);
}

__global__ __launch_bounds__(kCurveChunk) void curve_pitch_kernel(const CurveBatch b) {
    static_assert(kCurveChunk == 256, "four wave64 ballots cover a chunk");
    __shared__ float lg[kCurveChunk];
    __shared__ unsigned long long voiced_mask[4];
    const CurveD& c = b.c[b.pitch[blockIdx.x]];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int length = c.length;
    int carry_i = -1, gap = -1;         // the last voiced frame before this chunk; the first frame of a pending unvoiced run
    float carry_l = 0.f;
    for (int c0 = 0; c0 < length; c0 += kCurveChunk) {
        const int t = c0 + tid;
        const float v = t < length ? c.out[t] : 0.f;
        const bool voiced = t < length && v != 0.f;
        const float l = voiced ? (float)log2((double)v) : 0.f;
        lg[tid] = l;
        const unsigned long long m = __ballot(voiced);
        if (lane == 0) voiced_mask[wave] = m;
        __syncthreads();
        int fv = -1, lv = -1;           // first and last voiced frame of the chunk (uniform)
        for (int w = 0; w < 4; ++w) {
            const unsigned long long mw = voiced_mask[w];
            if (mw) {
                if (fv < 0) fv = w * 64 + __builtin_ctzll(mw);
                lv = w * 64 + 63 - __builtin_clzll(mw);
            }
        }
        if (gap >= 0 && fv >= 0) {      // the pending run ends at this chunk's first voiced frame
            const float nl = lg[fv];
            for (int u = gap + tid; u < c0; u += kCurveChunk)
                c.out[u] = pitch_finish(carry_i >= 0 ? pitch_between(u, carry_i, carry_l, c0 + fv, nl) : nl, b.log2_440);
        }
        if (voiced) {
            c.out[t] = pitch_finish(l, b.log2_440);
        } else if (t < length && fv >= 0 && tid < lv) {     // a voiced frame follows inside the chunk
            int p = -1, n = -1;
            for (int w = wave; w >= 0 && p < 0; --w) {
                unsigned long long mw = voiced_mask[w];
                if (w == wave) mw &= (1ull << lane) - 1ull;                 // lanes below this one
                if (mw) p = w * 64 + 63 - __builtin_clzll(mw);
            }
            for (int w = wave; w < 4 && n < 0; ++w) {
                unsigned long long mw = voiced_mask[w];
                if (w == wave) mw &= ~((1ull << lane) - 1ull);              // this lane (unvoiced: clear) and above
                if (mw) n = w * 64 + __builtin_ctzll(mw);
            }
            const int pi = p >= 0 ? c0 + p : carry_i;
            const float pl = p >= 0 ? lg[p] : carry_l;
            c.out[t] = pitch_finish(pi >= 0 ? pitch_between(t, pi, pl, c0 + n, lg[n]) : lg[n], b.log2_440);
        }
        if (fv >= 0) {
            carry_i = c0 + lv;
            carry_l = lg[lv];
            gap = c0 + lv + 1 < min(c0 + kCurveChunk, length) ? c0 + lv + 1 : -1;
        } else if (gap < 0) {
            gap = c0;
        }
        __syncthreads();                // lg and the masks are rewritten by the next chunk
    }
    if (gap >= 0) {
        const float tail = carry_i >= 0 ? pitch_finish(carry_l, b.log2_440) : -INFINITY;
        for (int u = gap + tid; u < length; u += kCurveChunk) c.out[u] = tail;
    }
}

const char* launch_curve_resample(const CurveBatch& b, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    curve_resample_kernel<<<dim3((b.max_pad + kCurveChunk - 1) / kCurveChunk, b.n), kCurveChunk, 0, st>>>(b);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && b.n_pitch > 0) {
        curve_pitch_kernel<<<dim3(b.n_pitch), kCurveChunk, 0, st>>>(b);
        e = hipGetLastError();
    }
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace dsd
