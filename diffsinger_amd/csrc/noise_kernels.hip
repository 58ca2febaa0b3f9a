// Seeded draws on the device (dsd_noise_fill): element (row, col) of stream s under (seed, domain) is a pure function of
// those five numbers - Philox4x32-10 on the counter (col >> 2, row, s, domain) with the seed as key - so a draw does not
// depend on the batch it is made in, on padding, or on the launch shape.  The specification is in include/dsdenoise.h.
//   noise_fill_kernel<VEC>   one thread = one Philox block = four consecutive columns of one row;
//                            out = src_scale * src + scale * eps, each product and the sum rounded on its own
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {

// VEC: cols % 4 == 0 and out (and src) 16-byte aligned - one 16-byte store (and load) per thread; otherwise scalar stores,
// which also cover the tail of a row.  The grid's x runs over (stream, row, column block), y over the launch's items.
template <bool VEC>
__global__ __launch_bounds__(256) void noise_fill_kernel(const NoiseP p) {
// a * src + b * eps stays two products and a sum: the seeded start mix of the samplers is then bitwise the one torch forms
// from the same eps, where a contracted fma would differ in the last bit
#pragma clang fp contract(off)
    const unsigned ncb = ((unsigned)p.cols + 3u) >> 2;
    const unsigned per = ncb * (unsigned)p.rows;                // <= elements of one item < 2^31 (host check)
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= per * (unsigned)p.n) return;
    const unsigned k = id / per, rem = id - k * per, r = rem / ncb, cb = rem - r * ncb;
    const unsigned long long seed = p.seed[blockIdx.y];
    const dsd_u32x4 w = philox4x32_10(dsd_u32x4{cb, r, p.first_stream + k, p.domain}, (unsigned)seed, (unsigned)(seed >> 32));
    float e[4];
    if (p.kind == 1) {
        e[0] = philox_uniform(w.x);
        e[1] = philox_uniform(w.y);
        e[2] = philox_uniform(w.z);
        e[3] = philox_uniform(w.w);
    } else {
        philox_normal2(w.x, w.y, e[0], e[1]);
        philox_normal2(w.z, w.w, e[2], e[3]);
    }
    const size_t base = (((size_t)k * p.B + (p.b0 + blockIdx.y)) * p.rows + r) * (size_t)p.cols + 4u * cb;
    if (VEC) {
        f32x4 v = {p.scale * e[0], p.scale * e[1], p.scale * e[2], p.scale * e[3]};
        if (p.src) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(p.src + base);
            v = p.src_scale * s + v;
        }
        *reinterpret_cast<f32x4*>(p.out + base) = v;
    } else {
        const int left = p.cols - (int)(4u * cb);               // >= 1
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) {
                float v = p.scale * e[i];
                if (p.src) v = p.src_scale * p.src[base + i] + v;
                p.out[base + i] = v;
            }
    }
}

hipError_t launch_noise_fill(const NoiseP& p, int items, hipStream_t st) {
    const unsigned threads = (unsigned)(((p.cols + 3) >> 2) * (long)p.rows * p.n);
    const dim3 grid((threads + 255u) / 256u, items);
    const bool vec = p.cols % 4 == 0 && ((uintptr_t)p.out & 15) == 0 && ((uintptr_t)p.src & 15) == 0;
    if (vec) noise_fill_kernel<true><<<grid, 256, 0, st>>>(p);
    else noise_fill_kernel<false><<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace dsd
