// Non-GEMM kernels of the NSF-HiFiGAN generator (mel + f0 -> waveform).  Every convolution
// with more than one input channel runs on the GEMM family of gemm.hip (transposed convolutions as phase-row GEMMs
// with a scatter epilogue); what is here is the harmonic-plus-noise source (SineGen / SourceModuleHnNSF), the
// single-input-channel strided "noise convs" that inject it at every resolution, and the residual-block average.
// Internal layout [batch][channel][Ts], lanes along time.
// RAG = 1 (dsd_vocode_ragged): item b of the batch is valid for lens[b] frames / samples of the launch's rate and is
// computed as if it had been run alone at that length; separate instantiations, so the dense kernels carry nothing new.
#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {
constexpr int kGroup = KG_VOCODER;      // whose create functions prepare this file's kernels (dsd_internal.h: KernelReg)

// ---------------------------------------------------------------------------------------------
// SineGen._f02sine, frame level (models.py:139-142): the phase each frame starts from is the running fp32 sum of
// the per-frame phase advances wrapped into [-0.5, 0.5) - torch.cumsum's sequential order, one lane per utterance.
//   rad_last = f0 / sr * upp;  rad2 = fmod(rad_last + 0.5, 1) - 0.5;  acc[t] = fmod(sum_{t' <= t} rad2[t'], 1)
// ---------------------------------------------------------------------------------------------
template <int RAG>
__global__ __launch_bounds__(256) void voc_phase_kernel(const float* __restrict__ f0, int T, float sr, int upp,
                                                        float* __restrict__ acc, const int* __restrict__ lens) {
    __shared__ float buf[2048];
    const int b = blockIdx.x;
    const int Tb = RAG ? lens[b] : T;              // the running phase of an item stops at its own end
    float run = 0.f;                               // carried by thread 0 across the 2048-frame pieces
    for (int base = 0; base < Tb; base += 2048) {
        const int n = min(2048, Tb - base);
        for (int i = threadIdx.x; i < n; i += 256) {       // per-frame advance, in parallel
            const float rad_last = f0[(long)b * T + base + i] / sr * (float)upp;
            buf[i] = fmodf(rad_last + 0.5f, 1.0f) - 0.5f;
        }
        __syncthreads();
        if (threadIdx.x == 0)                              // the running sum itself is sequential: same order as torch.cumsum
            for (int i = 0; i < n; ++i) {
                run += buf[i];
                buf[i] = fmodf(run, 1.0f);
            }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) acc[(long)b * T + base + i] = buf[i];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// SineGen.forward + SourceModuleHnNSF.forward, sample level (models.py:139-168, 200-203):
//   rad = f0/sr * (n+1) + acc[t-1];  per harmonic d: sin(2 pi (rad (d+1) + rand_ini[d])) * amp
//   sine * uv + (uv * noise_std + (1 - uv) * amp / 3) * noise  ->  tanh(Linear(dim -> 1))
// rand_ini [dim] (element 0 is forced to 0, models.py:146) and noise [B, T*upp, dim] are inputs: the reference
// draws them with torch.rand / torch.randn_like.
// ---------------------------------------------------------------------------------------------
// RAG = 1: rand_ini is [B][dim] (one draw per item, as B lone calls make them); samples past lens[b] * upp are not
// written (the noise convs read them as zero).
constexpr int VOC_MAXDIM = 16;
template <int RAG>
__global__ void voc_source_kernel(const float* __restrict__ f0, const float* __restrict__ acc,
                                  const float* __restrict__ rand_ini, const float* __restrict__ noise,
                                  const float* __restrict__ lin_w, const float* __restrict__ lin_b, int T, int upp,
                                  int dim, float sr, float sine_amp, float noise_std, int Tsu, float* __restrict__ har,
                                  const int* __restrict__ lens) {
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;       // sample index within the utterance
    if (s >= (long)(RAG ? lens[b] : T) * upp) return;
    if (RAG) rand_ini += (long)b * dim;
    const int t = (int)(s / upp), n = (int)(s - (long)t * upp);
    const float f = f0[(long)b * T + t];
    float rad = f / sr * (float)(n + 1);
    if (t > 0) rad += acc[(long)b * T + t - 1];
    const float uv = f > 0.f ? 1.f : 0.f;
    const float namp = uv * noise_std + (1.f - uv) * sine_amp / 3.f;
    const float* nz = noise + ((long)b * T * upp + s) * dim;
    float m = 0.f;
    for (int d = 0; d < dim; ++d) {
        float r = rad * (float)(d + 1);
        r += (d == 0) ? 0.f : rand_ini[d];
        const float sine = sinf(6.283185307179586f * r) * sine_amp;
        m += (sine * uv + namp * nz[d]) * lin_w[d];
    }
    har[(long)b * Tsu + s] = tanhf(m + lin_b[0]);
}

// ---------------------------------------------------------------------------------------------
// noise_convs[i] (models.py:239-245, 275-276): Conv1d(1, C, 2*sf, stride sf, padding sf/2) (or k = 1 at the last
// stage) on the source, ADDED to the upsampled activations:
//   x[b][o][q] += bias[o] + sum_k w[o][k] * har[b][q*sf - sf/2 + k]        (zero outside [0, Tup))
// Threads run along the output CHANNELS (weights are stored transposed, [k][C]: coalesced), every thread produces
// NQ consecutive frames of its channel, and the source window of the workgroup's frames sits in LDS, read as a
// broadcast.  One workgroup = min(C, 256) channels x (256 / C) groups of NQ frames.
// ---------------------------------------------------------------------------------------------
// The window is (groups * NQ - 1) * sf + ksz floats: thin stages far from the output rate (C = 16 at sf = 64: 65 792 bytes)
// outgrow the LDS, so the launch caps `groups` (voc_noise_groups) to what the raised limit holds and the threads of the
// groups cut away idle; a frame's sum does not depend on the group that forms it.
// RAG = 1: item b has lens_q[b] output frames and lens_up[b] source samples; a workgroup past its item's end returns.
constexpr int VOC_NQ = VOC_NOISE_NQ;
template <int RAG>
__global__ __launch_bounds__(256) void voc_noise_conv_kernel(float* __restrict__ x, const float* __restrict__ har,
                                                             const float* __restrict__ wt, const float* __restrict__ bias,
                                                             int C, int Tq, int Tsq, int sf, int ksz, long Tup, int Tsu,
                                                             int groups, const int* __restrict__ lens_q,
                                                             const int* __restrict__ lens_up) {
    extern __shared__ float win[];                  // (frames per workgroup - 1) * sf + ksz source samples
    const int b = blockIdx.z;
    const int cpb = C < 256 ? C : 256;              // channels per workgroup
    // groups: frame groups per workgroup, 256 / cpb or fewer (the launch's choice: voc_noise_groups)
    const int fpb = groups * VOC_NQ;                // frames per workgroup
    const int q0 = blockIdx.x * fpb;
    if (RAG) {
        Tq = lens_q[b];
        Tup = lens_up[b];
        if (q0 >= Tq) return;                       // whole workgroup: before the barrier
    }
    const int o = blockIdx.y * cpb + threadIdx.x % cpb, grp = threadIdx.x / cpb;
    const int pad = ksz > 1 ? sf / 2 : 0;
    const int nwin = (fpb - 1) * sf + ksz;
    const long s0 = (long)q0 * sf - pad;
    for (int i = threadIdx.x; i < nwin; i += 256) {
        const long sidx = s0 + i;
        win[i] = (sidx >= 0 && sidx < Tup) ? har[(long)b * Tsu + sidx] : 0.f;
    }
    __syncthreads();
    if (grp >= groups || o >= C) return;
    float acc[VOC_NQ];
#pragma unroll
    for (int j = 0; j < VOC_NQ; ++j) acc[j] = 0.f;
    const float* wbase = win + (grp * VOC_NQ) * sf;
    for (int k = 0; k < ksz; ++k) {
        const float w = wt[(long)k * C + o];
#pragma unroll
        for (int j = 0; j < VOC_NQ; ++j) acc[j] += w * wbase[j * sf + k];
    }
    const float bo = bias[o];
    float* xo = x + ((long)b * C + o) * Tsq + q0 + grp * VOC_NQ;
#pragma unroll
    for (int j = 0; j < VOC_NQ; ++j)
        if (q0 + grp * VOC_NQ + j < Tq) xo[j] += acc[j] + bo;
}

// acc = first ? r : acc + r;  if scale != 1: acc /= scale      (xs accumulation and `xs / num_kernels`, models.py:280-286)
__global__ void voc_accum_kernel(float* __restrict__ acc, const float* __restrict__ r, long n, int first, float div) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    f32x4 a = *reinterpret_cast<const f32x4*>(r + i);
    if (!first) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(acc + i);
        a = c + a;
    }
    if (div != 1.f) a = a / div;
    *reinterpret_cast<f32x4*>(acc + i) = a;
}

// ---------------------------------------------------------------------------------------------
// Generator.fastsinegen (models.py:251-260, mini_nsf): no harmonics, no noise; the per-sample phase advance is
// interpolated linearly towards the next frame's:
//   s0 = f0 / sr;  ds0 = s0[t+1] - s0[t] (0 at the last frame);  rad(n) = s0 n + 0.5 ds0 n (n - 1) / upp,  n = 1..upp
//   frame t starts from acc[t-1] = fmod(sum_{t' < t} (fmod(rad(upp) + 0.5, 1) - 0.5), 1);   out = sin(2 pi rad)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float voc_fast_rad(float s0, float ds0, int n, int upp) {
    const float fn = (float)n;
    return s0 * fn + 0.5f * ds0 * fn * (float)(n - 1) / (float)upp;
}

template <int RAG>
__global__ __launch_bounds__(256) void voc_fast_phase_kernel(const float* __restrict__ f0, int T, float sr, int upp,
                                                             float* __restrict__ acc, const int* __restrict__ lens) {
    __shared__ float buf[2048];
    const int b = blockIdx.x;
    const int Tb = RAG ? lens[b] : T;              // ds0 = 0 at the item's own last frame
    float run = 0.f;
    for (int base = 0; base < Tb; base += 2048) {
        const int n = min(2048, Tb - base);
        for (int i = threadIdx.x; i < n; i += 256) {
            const int t = base + i;
            const float s0 = f0[(long)b * T + t] / sr;
            const float ds0 = t + 1 < Tb ? f0[(long)b * T + t + 1] / sr - s0 : 0.f;
            buf[i] = fmodf(voc_fast_rad(s0, ds0, upp, upp) + 0.5f, 1.0f) - 0.5f;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i) {
                run += buf[i];
                buf[i] = fmodf(run, 1.0f);
            }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) acc[(long)b * T + base + i] = buf[i];
        __syncthreads();
    }
}

template <int RAG>
__global__ void voc_fast_source_kernel(const float* __restrict__ f0, const float* __restrict__ acc, int T, int upp, float sr,
                                       int Tsu, float* __restrict__ har, const int* __restrict__ lens) {
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Tb = RAG ? lens[b] : T;
    if (s >= (long)Tb * upp) return;
    const int t = (int)(s / upp), n = (int)(s - (long)t * upp) + 1;
    const float s0 = f0[(long)b * T + t] / sr;
    const float ds0 = t + 1 < Tb ? f0[(long)b * T + t + 1] / sr - s0 : 0.f;
    float rad = voc_fast_rad(s0, ds0, n, upp);
    if (t > 0) rad += acc[(long)b * T + t - 1];
    har[(long)b * Tsu + s] = sinf(6.283185307179586f * rad);
}

hipError_t launch_voc_fast_source(const float* f0, int B, int T, int upp, float source_sr, float* acc_tmp, int Tsu, float* har,
                                  hipStream_t st, const int* lens) {
    const long n = (long)T * upp;
    if (lens) {
        hipLaunchKernelGGL(voc_fast_phase_kernel<1>, dim3(B), dim3(256), 0, st, f0, T, source_sr, upp, acc_tmp, lens);
        hipLaunchKernelGGL(voc_fast_source_kernel<1>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, f0, acc_tmp, T,
                           upp, source_sr, Tsu, har, lens);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(voc_fast_phase_kernel<0>, dim3(B), dim3(256), 0, st, f0, T, source_sr, upp, acc_tmp, nullptr);
    hipLaunchKernelGGL(voc_fast_source_kernel<0>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, f0, acc_tmp, T, upp,
                       source_sr, Tsu, har, nullptr);
    return hipGetLastError();
}

hipError_t launch_voc_source(const float* f0, const float* rand_ini, const float* noise, const float* lin_w,
                             const float* lin_b, int B, int T, int upp, int dim, float sr, float sine_amp, float noise_std,
                             float* acc_tmp, int Tsu, float* har, hipStream_t st, const int* lens) {
    if (dim > VOC_MAXDIM) return hipErrorInvalidValue;
    const long n = (long)T * upp;
    if (lens) {
        hipLaunchKernelGGL(voc_phase_kernel<1>, dim3(B), dim3(256), 0, st, f0, T, sr, upp, acc_tmp, lens);
        hipLaunchKernelGGL(voc_source_kernel<1>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, f0, acc_tmp, rand_ini,
                           noise, lin_w, lin_b, T, upp, dim, sr, sine_amp, noise_std, Tsu, har, lens);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(voc_phase_kernel<0>, dim3(B), dim3(256), 0, st, f0, T, sr, upp, acc_tmp, nullptr);
    hipLaunchKernelGGL(voc_source_kernel<0>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, f0, acc_tmp, rand_ini, noise,
                       lin_w, lin_b, T, upp, dim, sr, sine_amp, noise_std, Tsu, har, nullptr);
    return hipGetLastError();
}

hipError_t launch_voc_noise_conv(float* x, const float* har, const float* w, const float* bias, int B, int C, int Tq,
                                 int Tsq, int sf, int ksz, long Tup, int Tsu, hipStream_t st, const int* lens_q,
                                 const int* lens_up) {
    const int groups = voc_noise_groups(C, sf, ksz);
    if (groups < 1) return hipErrorInvalidValue;    // not even one group's window fits (dsd_vocoder_create refuses these)
    const int cpb = C < 256 ? C : 256, fpb = groups * VOC_NQ;
    const int nwin = (fpb - 1) * sf + ksz;
    const dim3 grid((Tq + fpb - 1) / fpb, (C + cpb - 1) / cpb, B);
    // (the window is dynamic LDS beyond the default 64 KiB: the one kernel of this file that goes through the registry)
    if (lens_q)
        return launch_plain<voc_noise_conv_kernel<1>, kGroup>(grid, dim3(256), nwin * (int)sizeof(float), st, x, har, w, bias, C, Tq,
                                                              Tsq, sf, ksz, Tup, Tsu, groups, lens_q, lens_up);
    return launch_plain<voc_noise_conv_kernel<0>, kGroup>(grid, dim3(256), nwin * (int)sizeof(float), st, x, har, w, bias, C, Tq, Tsq,
                                                          sf, ksz, Tup, Tsu, groups, (const int*)nullptr, (const int*)nullptr);
}

// frame groups per workgroup of voc_noise_conv_kernel: one per min(C, 256) threads, fewer where the source window of that many
// would not fit the LDS the kernel may use; 0: not even one fits
int voc_noise_groups(int C, int sf, int ksz) {
    const int cpb = C < 256 ? C : 256;
    const long room = kMaxDynLds / (long)sizeof(float) - ksz;      // floats left for (groups * NQ - 1) * sf
    if (room < (long)(VOC_NQ - 1) * sf) return 0;
    const long fit = (room / sf + 1) / VOC_NQ;
    return (int)std::min<long>(256 / cpb, fit);
}

// x[row][t] += sigma * noise[row][t]  (models.py:272-273; x rows are padded to Ts, the caller's noise is dense)
// RAG = 1: item b (blockIdx.z) only over its lens[b] frames
template <int RAG>
__global__ void voc_add_noise_kernel(float* __restrict__ x, const float* __restrict__ noise, int T, int Ts, float sigma,
                                     const int* __restrict__ lens) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (RAG ? lens[blockIdx.z] : T)) return;
    const long row = (long)blockIdx.z * gridDim.y + blockIdx.y;
    x[row * Ts + t] += sigma * noise[row * T + t];
}

hipError_t launch_voc_add_noise(float* x, const float* noise, int B, int C, int T, int Ts, float sigma, hipStream_t st,
                                const int* lens) {
    if (lens)
        hipLaunchKernelGGL(voc_add_noise_kernel<1>, dim3((T + 255) / 256, C, B), dim3(256), 0, st, x, noise, T, Ts, sigma, lens);
    else
        hipLaunchKernelGGL(voc_add_noise_kernel<0>, dim3((T + 255) / 256, C, B), dim3(256), 0, st, x, noise, T, Ts, sigma, nullptr);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The seeded forms (dsd_vocode_seeded): the draws of voc_source_kernel and voc_add_noise_kernel made where they are used, so
// neither noise [B, T*upp, dim] nor pre_noise [B, C0, T] exists in memory.  Element (row, col) under an item's seed is the one
// dsd_noise_fill writes (noise_kernels.hip: counter (col >> 2, row, 0, domain), scale 1), and the arithmetic around it is the
// unseeded kernels' line for line, so the waveform is bit for bit the one of fill-then-vocode.  A launch covers up to
// kNoiseItems items from sd.b0; their seeds travel in the kernel arguments.
// ---------------------------------------------------------------------------------------------
template <int RAG>
__global__ void voc_source_seeded_kernel(const float* __restrict__ f0, const float* __restrict__ acc,
                                         const float* __restrict__ rand_ini, const float* __restrict__ lin_w,
                                         const float* __restrict__ lin_b, int T, int upp, int dim, float sr, float sine_amp,
                                         float noise_std, int Tsu, float* __restrict__ har, const int* __restrict__ lens,
                                         const VocSeedP sd) {
    const int b = sd.b0 + blockIdx.y;
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;       // sample index within the utterance: the draw's row
    if (s >= (long)(RAG ? lens[b] : T) * upp) return;
    if (RAG) rand_ini += (long)b * dim;
    const int t = (int)(s / upp), n = (int)(s - (long)t * upp);
    const float f = f0[(long)b * T + t];
    float rad = f / sr * (float)(n + 1);
    if (t > 0) rad += acc[(long)b * T + t - 1];
    const float uv = f > 0.f ? 1.f : 0.f;
    const float namp = uv * noise_std + (1.f - uv) * sine_amp / 3.f;
    const unsigned long long seed = sd.seed[blockIdx.y];
    float m = 0.f;
    for (int d0 = 0; d0 < dim; d0 += 4) {           // one Philox block per four harmonics, the last part-used
        const dsd_u32x4 w = philox4x32_10(dsd_u32x4{(unsigned)d0 >> 2, (unsigned)s, 0u, kVocSourceDomain}, (unsigned)seed,
                                          (unsigned)(seed >> 32));
        float nz[4];
        philox_normal2(w.x, w.y, nz[0], nz[1]);
        philox_normal2(w.z, w.w, nz[2], nz[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = d0 + i;
            if (d < dim) {
                float r = rad * (float)(d + 1);
                r += (d == 0) ? 0.f : rand_ini[d];
                const float sine = sinf(6.283185307179586f * r) * sine_amp;
                m += (sine * uv + namp * nz[i]) * lin_w[d];
            }
        }
    }
    har[(long)b * Tsu + s] = tanhf(m + lin_b[0]);
}

// x[row][t] += sigma * z(row = channel, col = t): one thread = one Philox block = four consecutive frames of one channel
template <int RAG>
__global__ void voc_add_noise_seeded_kernel(float* __restrict__ x, int T, int Ts, float sigma, const int* __restrict__ lens,
                                            const VocSeedP sd) {
    const int b = sd.b0 + blockIdx.z;
    const int Tb = RAG ? lens[b] : T;
    const int t0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (t0 >= Tb) return;
    const unsigned long long seed = sd.seed[blockIdx.z];
    const dsd_u32x4 w = philox4x32_10(dsd_u32x4{(unsigned)t0 >> 2, blockIdx.y, 0u, kVocPreDomain}, (unsigned)seed,
                                      (unsigned)(seed >> 32));
    float z[4];
    philox_normal2(w.x, w.y, z[0], z[1]);
    philox_normal2(w.z, w.w, z[2], z[3]);
    float* xr = x + ((long)b * gridDim.y + blockIdx.y) * Ts + t0;
    if (t0 + 4 <= Tb && (Ts & 3) == 0 && ((uintptr_t)x & 15) == 0) {
        f32x4 v = *reinterpret_cast<const f32x4*>(xr);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += sigma * z[i];
        *reinterpret_cast<f32x4*>(xr) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t0 + i < Tb) xr[i] += sigma * z[i];
    }
}

hipError_t launch_voc_source_seeded(const float* f0, const float* rand_ini, const unsigned long long* seeds, const float* lin_w,
                                    const float* lin_b, int B, int T, int upp, int dim, float sr, float sine_amp,
                                    float noise_std, float* acc_tmp, int Tsu, float* har, hipStream_t st, const int* lens) {
    if (dim > VOC_MAXDIM) return hipErrorInvalidValue;
    const long n = (long)T * upp;
    if (lens) hipLaunchKernelGGL(voc_phase_kernel<1>, dim3(B), dim3(256), 0, st, f0, T, sr, upp, acc_tmp, lens);
    else hipLaunchKernelGGL(voc_phase_kernel<0>, dim3(B), dim3(256), 0, st, f0, T, sr, upp, acc_tmp, nullptr);
    VocSeedP sd;
    for (int b0 = 0; b0 < B; b0 += kNoiseItems) {
        const int items = std::min(kNoiseItems, B - b0);
        sd.b0 = b0;
        for (int b = 0; b < kNoiseItems; ++b) sd.seed[b] = b < items ? seeds[b0 + b] : 0ull;
        const dim3 grid((unsigned)((n + 255) / 256), items);
        if (lens)
            hipLaunchKernelGGL(voc_source_seeded_kernel<1>, grid, dim3(256), 0, st, f0, acc_tmp, rand_ini, lin_w, lin_b, T, upp,
                               dim, sr, sine_amp, noise_std, Tsu, har, lens, sd);
        else
            hipLaunchKernelGGL(voc_source_seeded_kernel<0>, grid, dim3(256), 0, st, f0, acc_tmp, rand_ini, lin_w, lin_b, T, upp,
                               dim, sr, sine_amp, noise_std, Tsu, har, nullptr, sd);
    }
    return hipGetLastError();
}

hipError_t launch_voc_add_noise_seeded(float* x, const unsigned long long* seeds, int B, int C, int T, int Ts, float sigma,
                                       hipStream_t st, const int* lens) {
    VocSeedP sd;
    for (int b0 = 0; b0 < B; b0 += kNoiseItems) {
        const int items = std::min(kNoiseItems, B - b0);
        sd.b0 = b0;
        for (int b = 0; b < kNoiseItems; ++b) sd.seed[b] = b < items ? seeds[b0 + b] : 0ull;
        const dim3 grid(((T + 3) / 4 + 255) / 256, C, items);
        if (lens) hipLaunchKernelGGL(voc_add_noise_seeded_kernel<1>, grid, dim3(256), 0, st, x, T, Ts, sigma, lens, sd);
        else hipLaunchKernelGGL(voc_add_noise_seeded_kernel<0>, grid, dim3(256), 0, st, x, T, Ts, sigma, nullptr, sd);
    }
    return hipGetLastError();
}

hipError_t launch_voc_accum(float* acc, const float* r, long n, int first, float div, hipStream_t st) {
    hipLaunchKernelGGL(voc_accum_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, acc, r, n, first, div);
    return hipGetLastError();
}

}  // namespace dsd
