// The acoustic twin's stage kernels (dsd_acoustic_*, acoustic_api.hip): what deployment/modules/toplevel.py:61-81 and
// fastspeech2.py:59-130 write as torch ops around the encoder (masks, the gender -> key-shift and velocity -> speed
// arithmetic, f0_to_coarse), the start state of the two samplers (diffusion.py:117-129, rectified_flow.py:45-56) and
// ensure_mel_base.  Plain launches outside the kernel registry, as stage_kernels.hip's: all are latency-bound on small
// grids.  Every fp32 operation here is one torch rounds on its own, so the file's contraction is switched off and the
// arithmetic is written with plain operators: hipcc contracts a * b + c into an FMA by default, and does so through
// __fmul_rn / __fadd_rn too (inline functions of HIP's headers, compiled with contraction on; seen in the ISA).  The
// division is the correctly rounded __fdiv_rn.  The outputs are then bit-identical to the Python twin's
// (diffsinger_amd/deploy.py) on the same operands.
#include "dsd_internal.h"
#include "dsd_device.h"

#pragma clang fp contract(off)

namespace dsd {

// ---------------------------------------------------------------------------------------------
// Per token l of item b, lanes along the tokens:
//   dur_m[l] = durations[l] * (tokens[l] > 0)
//   lang[l]  = languages[l] * mask[tokens[l]]   (_masked_languages); languages == nullptr: 0 (a multilingual model whose
//              cross-lingual list is empty: every token takes lang_embed's padding row)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ac_tokens_kernel(const AcTokensP p) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= p.L) return;
    const long i = (long)b * p.L + l;
    const long long tok = p.tokens[i];
    p.dur_m[i] = tok > 0 ? p.durations[i] : 0;
    if (p.lang) {
        long long lang = 0;
        if (p.languages) {
            const bool cross = tok >= 0 && tok < p.vocab && p.mask[tok] != 0.f;
            lang = cross ? p.languages[i] : 0;
        }
        p.lang[i] = lang;
    }
}

hipError_t launch_ac_tokens(const AcTokensP& p, int B, hipStream_t st) {
    ac_tokens_kernel<<<dim3((p.L + 255) / 256, B), 256, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Per frame t of item b, lanes along the frames:
//   f0_m      = f0 * (mel2ph > 0)                                          (a product, as the twin's: an infinite f0 on a
//                                                                           padding frame gives NaN there too)
//   f0_enc    = f0_m, or 0 with the discrete embedding (the encoder's Linear(1, H) pitch term is stored as zeros)
//   key_shift = frozen[0], or with g = clip(gender, -1, 1), m = g < 0:  g * ((1 - m) * shift_max + m * |shift_min|)
//   speed     = clip(velocity, speed_min, speed_max), or 1
//   iota      = t                                                          (the gather of the condition at its own rows)
//   coarse    = f0_to_coarse(f0_m) (fastspeech2.py:21-28), operation by operation as torch runs it on the device:
//               f0 / 700 is a product with fp32(1 / 700) (a division by a host scalar), 1 + x, logf, 1127 * x, then where
//               (mel > 0): mel * fp32(a) - fp32(b), clip to [1, 255] (a NaN stays one and converts as torch's .long() does
//               on the device), round half to even
// torch.clip passes a NaN through: the comparisons below do too.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ac_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(256) void ac_frames_kernel(const AcFramesP p) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= p.T) return;
    const long i = (long)b * p.T + t;
    const float f0 = p.f0[i] * (p.mel2ph[i] > 0 ? 1.f : 0.f);
    p.f0_m[i] = f0;
    if (p.f0_enc) p.f0_enc[i] = p.coarse ? 0.f : f0;
    if (p.key_shift) {
        float ks;
        if (p.frozen_key_shift) {
            ks = p.frozen_key_shift[0];
        } else {
            const float g = ac_clip(p.gender[i], -1.f, 1.f);
            const float m = g < 0.f ? 1.f : 0.f;
            const float up = (1.f - m) * p.shift_max, down = m * p.shift_min_abs;
            ks = g * (up + down);
        }
        p.key_shift[i] = ks;
    }
    if (p.speed) p.speed[i] = p.velocity ? ac_clip(p.velocity[i], p.speed_min, p.speed_max) : 1.f;
    if (p.iota) p.iota[i] = t;
    if (p.coarse) {
        const float ratio = f0 * p.inv_700;
        float mel = 1127.f * logf(1.f + ratio);
        if (mel > 0.f) mel = mel * p.coarse_a - p.coarse_b;
        mel = ac_clip(mel, 1.f, 255.f);
        const long long c = (long long)rintf(mel);
        p.coarse[i] = c;
        if (p.coarse_out) p.coarse_out[i] = c;
    }
}

hipError_t launch_ac_frames(const AcFramesP& p, int B, hipStream_t st) {
    ac_frames_kernel<<<dim3((p.T + 255) / 256, B), 256, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The samplers' start state: source [B][T][M] -> x [B][1][M][T],
//   x[b][m][t] = (source[b][t][m] - mid[m]) / k[m]                                   (norm_spec, a correctly rounded division)
//   x[b][m][t] = src_scale * that + noise_scale * noise[b][m][t]    with `noise`     (q_sample / the reflow mix: two products
//                                                                                     and a sum, each rounded on its own)
// An LDS-tiled transpose: a 32 x 32 tile per workgroup of 32 x 8 lanes; the loads run along M (threadIdx.x) and normalise
// with the lane's own k[m] and mid[m], the stores - and the noise loads - run along T.  The tile's rows are 33 words long:
// a row read (ds_read_b32, banks = word address mod 32, conflicts counted per 32-lane half) walks 32 consecutive rows at one
// column, 33 words apart, and so 32 different banks; the writes of a half are 32 consecutive words.  Edge tiles are masked on
// both sides, so any M >= 1 and T >= 1 works.
// ---------------------------------------------------------------------------------------------
constexpr int kAcTile = 32;

__global__ __launch_bounds__(256) void ac_source_kernel(const float* __restrict__ source, const float* __restrict__ noise,
                                                        const float* __restrict__ k, const float* __restrict__ mid, float src_scale,
                                                        float noise_scale, int M, int T, float* __restrict__ x) {
    __shared__ float tile[kAcTile][kAcTile + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, b = blockIdx.z;
    const int t0 = blockIdx.x * kAcTile, m0 = blockIdx.y * kAcTile;
    {
        const int m = m0 + tx;
        if (m < M) {
            const float km = k[m], bm = mid[m];
            const float* src = source + (long)b * T * M + m;
#pragma unroll
            for (int j = 0; j < kAcTile; j += 8) {
                const int t = t0 + ty + j;
                if (t < T) tile[ty + j][tx] = __fdiv_rn(src[(long)t * M] - bm, km);
            }
        }
    }
    __syncthreads();
    const int t = t0 + tx;
    if (t >= T) return;
#pragma unroll
    for (int j = 0; j < kAcTile; j += 8) {
        const int m = m0 + ty + j;
        if (m >= M) break;
        const long o = ((long)b * M + m) * T + t;
        float v = tile[tx][ty + j];
        if (noise) v = src_scale * v + noise_scale * noise[o];
        x[o] = v;
    }
}

hipError_t launch_ac_source(const float* source, const float* noise, const float* k, const float* mid, float src_scale, float noise_scale,
                            int B, int M, int T, float* x, hipStream_t st) {
    ac_source_kernel<<<dim3((T + kAcTile - 1) / kAcTile, (M + kAcTile - 1) / kAcTile, B), dim3(kAcTile, 8), 0, st>>>(
        source, noise, k, mid, src_scale, noise_scale, M, T, x);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// ensure_mel_base (toplevel.py:55-59): mel *= scale in place.  16 bytes per lane when the count is a multiple of 4 and the
// pointer 16-byte aligned (the launcher decides), one float per lane otherwise.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ac_mel_base_kernel(float* __restrict__ mel, long n, float scale, int vec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        if (i * 4 >= n) return;
        float4 v = reinterpret_cast<float4*>(mel)[i];
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        reinterpret_cast<float4*>(mel)[i] = v;
    } else {
        if (i >= n) return;
        mel[i] *= scale;
    }
}

hipError_t launch_ac_mel_base(float* mel, long n, float scale, hipStream_t st) {
    const int vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(mel) & 15) == 0;
    const long lanes = vec ? n / 4 : n;
    ac_mel_base_kernel<<<dim3((unsigned)((lanes + 255) / 256)), 256, 0, st>>>(mel, n, scale, vec);
    return hipGetLastError();
}

}  // namespace dsd
