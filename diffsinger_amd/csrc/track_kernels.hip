// A project's track on the device (dsd_track_place / dsd_track_peak / dsd_track_export; the semantics are in
// include/dsdenoise.h): three elementwise, memory-bound kernels over a float64 track.
//   track_place_kernel    the gap's zeros, the cross-fade and the copy of one segment, in one launch
//   track_peak_kernel     max |v| as the maximum of the bit patterns, one vector atomic per workgroup
//   track_export_kernel   float64 copy, fp32, or save_wav's int16
// All three index the work by TRACK position: a workgroup covers kTrackSpan consecutive samples, a thread the 16-byte
// aligned pair of doubles at (base + 2 * thread), where base is the first sample at or below the range whose address is
// 16-byte aligned.  A pair that lies wholly inside the range moves as one 16-byte access; the ragged first and last sample
// of the range take the 8-byte one.  A segment's start is arbitrary, so src is read 4 bytes at a time at whatever alignment
// falls out (consecutive lanes read consecutive pairs: the wave still reads one contiguous run).  Sample indices are
// 64-bit throughout.
//
// The blend and the PCM scaling are numpy's operations one by one - (1 - r) * a + r * b is two products and a sum, each
// rounded to float64 - so nothing here may be contracted into an fma: contraction is off for the whole file.
#pragma clang fp contract(off)
#include "dsd_internal.h"
#include "../../include/dsdenoise.h"

namespace dsd {

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
constexpr int kTrackThreads = kTrackSpan / 2;
static_assert(kTrackThreads == 256, "one pair of doubles per thread of a 256-thread workgroup");

// the first index <= lo whose double is 16-byte aligned (it may be lo - 1, hence -1: never accessed)
inline long long pair_base(const double* track, long long lo) {
    const long long odd = (long long)(((uintptr_t)track >> 3) & 1);      // track[odd] is the first aligned sample
    return lo - ((lo + odd) & 1);
}
inline unsigned span_blocks(long long base, long long hi) { return (unsigned)((hi - base + kTrackSpan - 1) / kTrackSpan); }

struct PlaceP {
    double* track;
    const float* src;
    long long base;         // pair_base(track, lo)
    long long lo, hi;       // the samples this call writes: [min(prev_end, start), start + n)
    long long s, p;         // start, prev_end
    long long F;            // p - s: > 0 overlap, <= 0 gap
    double step;            // 1.0 / (F - 1) for F > 1 (np.linspace's step, divided on the host in double), else 0
};

// sample i of [lo, hi) after the call; `old` is track[i], read only inside the fade
__device__ __forceinline__ double place_value(const PlaceP& q, long long i, double old) {
    if (i < q.s) return 0.0;                                    // the gap [p, s)
    const long long j = i - q.s;
    const double w = (double)q.src[j];
    if (i >= q.p) return w;                                     // the copy [max(p, s), s + n)
    const double r = (j == q.F - 1 && q.F > 1) ? 1.0 : (double)j * q.step;         // linspace(0, 1, F): the end point is exact
    return (1.0 - r) * old + r * w;
}

__global__ __launch_bounds__(kTrackThreads) void track_place_kernel(const PlaceP q) {
    const long long i0 = q.base + 2 * ((long long)blockIdx.x * kTrackThreads + threadIdx.x), i1 = i0 + 1;
    const bool in0 = i0 >= q.lo && i0 < q.hi, in1 = i1 >= q.lo && i1 < q.hi;
    if (!in0 && !in1) return;
    const bool fade0 = in0 && i0 >= q.s && i0 < q.p, fade1 = in1 && i1 >= q.s && i1 < q.p;
    double a0 = 0.0, a1 = 0.0;
    if (fade0 && fade1) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(q.track + i0);
        a0 = a.x;
        a1 = a.y;
    } else if (fade0) {
        a0 = q.track[i0];                                       // the fade's last sample shares its pair with the copy
    } else if (fade1) {
        a1 = q.track[i1];                                       // the fade's first sample: the one before it is not ours
    }
    if (in0 && in1) {
        const f64x2 v = {place_value(q, i0, a0), place_value(q, i1, a1)};
        *reinterpret_cast<f64x2*>(q.track + i0) = v;
    } else if (in0) {
        q.track[i0] = place_value(q, i0, a0);                   // ragged tail of the range
    } else {
        q.track[i1] = place_value(q, i1, a1);                   // ragged head
    }
}

// |v| as an unsigned integer: for non-negative doubles the order of the bit patterns is the order of the values, and every
// NaN sorts above infinity, so a NaN sample comes out as a NaN (np.abs(x).max() propagates it too)
__device__ __forceinline__ unsigned long long abs_bits(double v) {
    return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
}

__global__ __launch_bounds__(kTrackThreads) void track_peak_kernel(const double* __restrict__ track, long long base, long long total,
                                                                   unsigned long long* peak_bits) {
    __shared__ unsigned long long part[kTrackThreads];
    const long long i0 = base + 2 * ((long long)blockIdx.x * kTrackThreads + threadIdx.x), i1 = i0 + 1;
    const bool in0 = i0 >= 0 && i0 < total, in1 = i1 < total;           // i1 >= 0 always
    unsigned long long m = 0;
    if (in0 && in1) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(track + i0);
        const unsigned long long x = abs_bits(a.x), y = abs_bits(a.y);
        m = x > y ? x : y;
    } else if (in0) {
        m = abs_bits(track[i0]);
    } else if (in1) {
        m = abs_bits(track[i1]);
    }
    part[threadIdx.x] = m;
    __syncthreads();
    for (int half = kTrackThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            const unsigned long long o = part[threadIdx.x + half];
            if (o > part[threadIdx.x]) part[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0] != 0) atomicMax(peak_bits, part[0]);
}

// save_wav: (v / peak) * 32767 or v * 32767 in float64, then astype(np.int16) = truncation toward zero.  Outside int16 the
// value saturates and NaN gives 0 (numpy: undefined); a zero peak gives 0 (numpy: 0 / 0)
__device__ __forceinline__ short pcm_value(double v, bool norm, double peak) {
    double x;
    if (norm) x = peak == 0.0 ? 0.0 : (v / peak) * 32767.0;
    else x = v * 32767.0;
    if (x != x) return 0;
    if (x <= -32768.0) return (short)-32768;
    if (x >= 32767.0) return (short)32767;
    return (short)(int)x;
}

template <int KIND> struct ExportOut;
template <> struct ExportOut<DSD_TRACK_F64> { typedef double T; typedef f64x2 T2; };
template <> struct ExportOut<DSD_TRACK_F32> { typedef float T; typedef f32x2 T2; };
template <> struct ExportOut<DSD_TRACK_PCM> { typedef short T; typedef i16x2 T2; };

// pair_out: out + i0 is aligned for a two-element store wherever track + i0 is 16-byte aligned (host check)
template <int KIND>
__global__ __launch_bounds__(kTrackThreads) void track_export_kernel(const double* __restrict__ track, long long base, long long total,
                                                                     const double* __restrict__ peak, void* out_, bool pair_out) {
    typedef typename ExportOut<KIND>::T T;
    typedef typename ExportOut<KIND>::T2 T2;
    T* out = static_cast<T*>(out_);
    const long long i0 = base + 2 * ((long long)blockIdx.x * kTrackThreads + threadIdx.x), i1 = i0 + 1;
    const bool in0 = i0 >= 0 && i0 < total, in1 = i1 < total;
    if (!in0 && !in1) return;
    const bool norm = KIND == DSD_TRACK_PCM && peak != nullptr;
    const double pk = norm ? *peak : 0.0;
    double a0 = 0.0, a1 = 0.0;
    if (in0 && in1) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(track + i0);
        a0 = a.x;
        a1 = a.y;
    } else if (in0) {
        a0 = track[i0];
    } else {
        a1 = track[i1];
    }
    T v0, v1;
    if (KIND == DSD_TRACK_PCM) {
        v0 = (T)pcm_value(a0, norm, pk);
        v1 = (T)pcm_value(a1, norm, pk);
    } else {
        v0 = (T)a0;                                             // fp32: one rounding to nearest even
        v1 = (T)a1;
    }
    if (in0 && in1 && pair_out) {
        const T2 v = {v0, v1};
        *reinterpret_cast<T2*>(out + i0) = v;
    } else {
        if (in0) out[i0] = v0;
        if (in1) out[i1] = v1;
    }
}

inline const char* last_launch_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace

// the callers (track_api.hip) have checked the geometry: 0 <= start, n >= 1, 0 <= prev_end <= start + n <= total
const char* launch_track_place(double* track, long long start, long long prev_end, const float* src, long long n, void* stream) {
    PlaceP q;
    q.track = track;
    q.src = src;
    q.s = start;
    q.p = prev_end;
    q.F = prev_end - start;
    q.lo = prev_end < start ? prev_end : start;
    q.hi = start + n;
    q.base = pair_base(track, q.lo);
    q.step = q.F > 1 ? 1.0 / (double)(q.F - 1) : 0.0;
    track_place_kernel<<<span_blocks(q.base, q.hi), kTrackThreads, 0, (hipStream_t)stream>>>(q);
    return last_launch_error();
}

const char* launch_track_peak(const double* track, long long total, double* peak_out, void* stream) {
    const hipError_t e = hipMemsetAsync(peak_out, 0, sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return hipGetErrorString(e);
    const long long base = pair_base(track, 0);
    track_peak_kernel<<<span_blocks(base, total), kTrackThreads, 0, (hipStream_t)stream>>>(
        track, base, total, reinterpret_cast<unsigned long long*>(peak_out));
    return last_launch_error();
}

const char* launch_track_export(const double* track, long long total, int kind, const double* peak, void* out, void* stream) {
    const long long base = pair_base(track, 0);
    const unsigned blocks = span_blocks(base, total);
    const hipStream_t st = (hipStream_t)stream;
    // a pair starts at an index of base's parity: out + that index must be aligned to two elements
    const size_t elem = kind == DSD_TRACK_F64 ? 8 : kind == DSD_TRACK_F32 ? 4 : 2;
    const bool pair_out = (((uintptr_t)out + (size_t)(base & 1) * elem) & (2 * elem - 1)) == 0;
    if (kind == DSD_TRACK_F64) track_export_kernel<DSD_TRACK_F64><<<blocks, kTrackThreads, 0, st>>>(track, base, total, peak, out, pair_out);
    else if (kind == DSD_TRACK_F32) track_export_kernel<DSD_TRACK_F32><<<blocks, kTrackThreads, 0, st>>>(track, base, total, peak, out, pair_out);
    else track_export_kernel<DSD_TRACK_PCM><<<blocks, kTrackThreads, 0, st>>>(track, base, total, peak, out, pair_out);
    return last_launch_error();
}

}  // namespace dsd
