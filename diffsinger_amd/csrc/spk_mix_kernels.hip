// Speaker mixes on the device (dsd_acoustic_spk_mix, dsd_variance_spk_mix): what the inference front ends write as
// `torch.sum(spk_embed(ids) * values, dim=2)` (inference/ds_acoustic.py:191-197, ds_variance.py:315-326), for a caller who
// holds the model file and cannot read the table back.
//   out[b, r, h] = sum over n = 0 .. N-1, in that order, of w[b, r, n] * table[ids[b, n], h]
//   w = values, or with normalize: values / s, s = values[b, r, 0] + values[b, r, 1] + ... in index order
// Every product, sum and the division (__fdiv_rn) is rounded to fp32 on its own, so the file's contraction is off, as in
// acoustic_kernels.hip.  A plain launch outside the kernel registry: latency-bound, no LDS.
//   spk_mix_kernel<VEC>   lanes along H - VEC: four columns (16 bytes) per lane - and `lanes` of them per (b, r) row, 256 / lanes
//                         rows per workgroup.  A row's N weights are read by its lanes at one address per step (one broadcast
//                         load per wave), the speaker ids likewise.
#include "dsd_internal.h"
#include "dsd_device.h"

#pragma clang fp contract(off)

namespace dsd {

template <bool VEC>
__global__ __launch_bounds__(256) void spk_mix_kernel(const SpkMixP p) {
    const int rpb = 256 / p.lanes;
    const int r = blockIdx.x * rpb + (int)threadIdx.x / p.lanes, lane = (int)threadIdx.x % p.lanes, b = blockIdx.y;
    if (r >= p.rows) return;
    const float* v = p.values + ((long)b * p.rows + r) * p.N;
    const int* id = p.ids + (long)b * p.N;
    float s = 1.f;
    if (p.normalize) {
        s = v[0];
        for (int n = 1; n < p.N; ++n) s = s + v[n];
    }
    float* o = p.out + ((long)b * p.rows + r) * p.H;
    if (VEC) {
        for (int j = lane; j < p.H / 4; j += p.lanes) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int n = 0; n < p.N; ++n) {
                const float w = p.normalize ? __fdiv_rn(v[n], s) : v[n];
                const f32x4 e = *reinterpret_cast<const f32x4*>(p.table + (long)id[n] * p.H + 4 * j);
                const f32x4 t = w * e;
                acc = n == 0 ? t : acc + t;
            }
            *reinterpret_cast<f32x4*>(o + 4 * j) = acc;
        }
    } else {
        for (int j = lane; j < p.H; j += p.lanes) {
            float acc = 0.f;
            for (int n = 0; n < p.N; ++n) {
                const float w = p.normalize ? __fdiv_rn(v[n], s) : v[n];
                const float t = w * p.table[(long)id[n] * p.H + j];
                acc = n == 0 ? t : acc + t;
            }
            o[j] = acc;
        }
    }
}

hipError_t launch_spk_mix(SpkMixP p, int B, hipStream_t st) {
    const bool vec = p.H % 4 == 0 && ((uintptr_t)p.table & 15) == 0 && ((uintptr_t)p.out & 15) == 0;
    const int cols = vec ? p.H / 4 : p.H;
    p.lanes = 1;
    while (p.lanes < cols && p.lanes < 256) p.lanes *= 2;       // a power of two: 256 / lanes whole rows per workgroup
    const int rpb = 256 / p.lanes;
    const dim3 grid((p.rows + rpb - 1) / rpb, B);
    if (vec) hipLaunchKernelGGL(spk_mix_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(spk_mix_kernel<false>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace dsd
