// Validation scoring (dsd_diffuse, dsd_masked_loss, dsd_curve_stats, dsd_dur_score): the noising step of p_losses and the
// reductions of the reference's losses and metrics.  The specification - what a term is, what is fp32 and what is double,
// the order of the sums - is in include/dsdenoise.h above DSD_SCORE_WORKSPACE_BYTES.
//   diffuse_kernel<VEC>       one thread = four consecutive columns of one row (the Philox block of noise_fill_kernel)
//   loss_kernel, curve_kernel, dur_terms_kernel
//                             per-workgroup partial sums of a reduction: [kScoreSlots][kScoreMaxBlocks] in the workspace
//   score_final_kernel<KIND>  one workgroup: adds the partials in a fixed order and writes the result
//   dur_words_kernel          one thread per (item, word): the word sums in phoneme order
#include "../../include/dsdenoise.h"
#include "dsd_internal.h"
#include "dsd_device.h"

// every product and sum below stays an operation of its own: a term is then bitwise what the reference's fp32 ops give,
// where a contracted fma would differ in the last bit (as in noise_kernels.hip)
#pragma clang fp contract(off)

namespace dsd {
namespace {

// ---------------------------------------------------------------------------------------------
// dsd_diffuse
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void diffuse_kernel(const DiffuseP p) {
    const unsigned ncb = ((unsigned)p.cols + 3u) >> 2;
    const unsigned per = ncb * (unsigned)p.rows;                // <= elements of one item < 2^31 (host check)
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= per) return;
    const unsigned r = id / ncb, cb = id - r * ncb;
    const int b = p.b0 + (int)blockIdx.y;
    const size_t base = ((size_t)b * p.rows + r) * (size_t)p.cols + 4u * cb;
    const int left = VEC ? 4 : min(4, p.cols - (int)(4u * cb)); // >= 1
    float e[4] = {0.f, 0.f, 0.f, 0.f}, x[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.eps) {
        if (VEC) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p.eps + base);
            e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < left) e[i] = p.eps[base + i];
        }
    } else {        // dsd_noise_fill's draw at (seed, domain, stream 0, r, 4 cb + i), DSD_NOISE_NORMAL
        const unsigned long long seed = p.seed[blockIdx.y];
        const dsd_u32x4 w = philox4x32_10(dsd_u32x4{cb, r, 0u, p.domain}, (unsigned)seed, (unsigned)(seed >> 32));
        philox_normal2(w.x, w.y, e[0], e[1]);
        philox_normal2(w.z, w.w, e[2], e[3]);
    }
    if (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.x0 + base);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) x[i] = p.x0[base + i];
    }
    const float a = p.a[b];
    float xt[4], tg[4];
    if (p.kind == DSD_DIFFUSE_DDPM) {       // q_sample, ddpm.py:206-210
        const float c = p.c[b];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ax = a * x[i], ce = c * e[i];
            xt[i] = ax + ce;
            tg[i] = e[i];
        }
    } else {                                // reflow.py:38,41
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tg[i] = x[i] - e[i];
            const float at = a * tg[i];
            xt[i] = e[i] + at;
        }
    }
    if (VEC) {
        *reinterpret_cast<f32x4*>(p.x_t + base) = f32x4{xt[0], xt[1], xt[2], xt[3]};
        if (p.target) *reinterpret_cast<f32x4*>(p.target + base) = f32x4{tg[0], tg[1], tg[2], tg[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) {
                p.x_t[base + i] = xt[i];
                if (p.target) p.target[base + i] = tg[i];
            }
    }
}

// ---------------------------------------------------------------------------------------------
// The reductions: three double and four integer sums per launch (slots 0-2 and 3-6 of the workspace)
// ---------------------------------------------------------------------------------------------
constexpr int kAccD = 3, kAccI = 4;
static_assert(kAccD + kAccI <= kScoreSlots, "one workspace slot per sum");
struct Acc {
    double d[kAccD];
    long long i[kAccI];
};

// sum over the workgroup in a fixed order: i with i + 128, then + 64, ... + 1; every thread returns the total
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int half = kScoreThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) sh[threadIdx.x] += sh[threadIdx.x + half];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// the spans blockIdx.x, + gridDim.x, ... of kScoreSpan elements; term(e, acc) adds element e < n < 2^31
template <typename F>
__device__ __forceinline__ void score_partials(unsigned n, void* ws, F&& term) {
    __shared__ double shd[kScoreThreads];
    __shared__ long long shi[kScoreThreads];
    Acc a;
    for (int j = 0; j < kAccD; ++j) a.d[j] = 0.0;
    for (int j = 0; j < kAccI; ++j) a.i[j] = 0;
    const unsigned spans = (n + (unsigned)kScoreSpan - 1u) / (unsigned)kScoreSpan;
    for (unsigned s = blockIdx.x; s < spans; s += gridDim.x) {
        const unsigned e0 = s * (unsigned)kScoreSpan + threadIdx.x;     // < 2^31 + kScoreSpan
        for (int k = 0; k < kScoreSpan / kScoreThreads; ++k) {
            const unsigned e = e0 + (unsigned)(k * kScoreThreads);
            if (e < n) term(e, a);
        }
    }
    double* wd = static_cast<double*>(ws);
    long long* wi = static_cast<long long*>(ws);
    for (int j = 0; j < kAccD; ++j) {
        const double r = block_sum(a.d[j], shd);
        if (threadIdx.x == 0) wd[j * kScoreMaxBlocks + blockIdx.x] = r;
    }
    for (int j = 0; j < kAccI; ++j) {
        const long long r = block_sum(a.i[j], shi);
        if (threadIdx.x == 0) wi[(kAccD + j) * kScoreMaxBlocks + blockIdx.x] = r;
    }
}

// reflow_loss.py:26-34 in double from the fp32 t
__device__ __forceinline__ double lognorm_weight(float t32) {
    double t = (double)t32;
    t = t < 1e-7 ? 1e-7 : (t > 1.0 - 1e-7 ? 1.0 - 1e-7 : t);          // a NaN stays one, as torch.clip keeps it
    const double l = log(t / (1.0 - t));
    return 0.398942 / t / (1.0 - t) * exp(-0.5 * (l * l)) + 1e-7;
}

__global__ __launch_bounds__(kScoreThreads) void loss_kernel(const LossP p, unsigned n, void* ws) {
    const unsigned rc = (unsigned)p.rows * (unsigned)p.cols;
    int cur_b = -1;
    double w = 1.0;
    score_partials(n, ws, [&](unsigned e, Acc& a) {
        const unsigned b = e / rc, col = (e - b * rc) % (unsigned)p.cols;
        float x = p.pred[e], y = p.target[e];
        if (p.non_padding) {
            const float m = p.non_padding[(size_t)b * p.cols + col];
            x = x * m;
            y = y * m;
        }
        const float d = x - y;
        const float term = p.kind == DSD_LOSS_L1 ? fabsf(d) : d * d;
        if (p.t) {
            if ((int)b != cur_b) {          // once per item and thread: a thread's elements change item rarely
                cur_b = (int)b;
                w = lognorm_weight(p.t[b]);
            }
            a.d[0] += (double)term * w;
        } else {
            a.d[0] += (double)term;
        }
    });
}

__global__ __launch_bounds__(kScoreThreads) void curve_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                              const unsigned char* __restrict__ mask, unsigned n, float tol, void* ws) {
    score_partials(n, ws, [&](unsigned e, Acc& a) {
        if (mask && !mask[e]) return;
        const float x = pred[e], y = target[e];
        const float d = x - y, r = y - x;
        a.i[0] += fabsf(d) <= tol ? 1 : 0;
        a.i[1] += 1;
        a.d[0] += (double)y;
        a.d[1] += (double)(y * y);
        a.d[2] += (double)(r * r);
    });
}

__device__ __forceinline__ float clamp0(float v) { return v < 0.f ? 0.f : v; }     // a NaN stays one (torch.clamp)

// nn.MSELoss / nn.HuberLoss (delta 1) on log(x + offset) - log(y + offset), the sums fp32, the logs double
__device__ __forceinline__ double dur_term(float x, float y, float offset, int kind) {
    const float xo = x + offset, yo = y + offset;
    const double d = log((double)xo) - log((double)yo);
    if (kind == DSD_DUR_MSE) return d * d;
    const double ad = fabs(d);
    return ad < 1.0 ? 0.5 * (d * d) : ad - 0.5;
}

__global__ __launch_bounds__(kScoreThreads) void dur_words_kernel(const DurP p) {
    const unsigned id = blockIdx.x * (unsigned)kScoreThreads + threadIdx.x;
    if (id >= (unsigned)p.B * (unsigned)p.n_words) return;
    const unsigned b = id / (unsigned)p.n_words;
    const long long w = id - b * (unsigned)p.n_words;
    if (w == 0) return;                                         // padding: [:, 1:] drops it
    const size_t row = (size_t)b * p.L;
    float sp = 0.f, sg = 0.f;
    for (int l = 0; l < p.L; ++l)
        if (p.ph2word[row + l] == w) {
            sp += clamp0(p.dur_pred[row + l]);
            sg += p.dur_gt[row + l];
        }
    const size_t o = (size_t)b * (p.n_words - 1) + (size_t)(w - 1);
    p.wdur_pred[o] = sp;
    p.wdur_gt[o] = sg;
}

// elements: B * L phonemes, then B * (n_words - 1) words, then B items
__global__ __launch_bounds__(kScoreThreads) void dur_terms_kernel(const DurP p, unsigned n, void* ws) {
    const unsigned nph = (unsigned)p.B * (unsigned)p.L, nwd = (unsigned)p.B * (unsigned)(p.n_words - 1);
    const unsigned W1 = (unsigned)(p.n_words - 1);
    score_partials(n, ws, [&](unsigned e, Acc& a) {
        if (e < nph) {
            const unsigned b = e / (unsigned)p.L;
            const float x = p.dur_pred[e], y = p.dur_gt[e];
            a.d[0] += dur_term(x, y, p.offset, p.kind);         // on the unclamped prediction (dur_loss.py:34)
            // RhythmRegulator (tts_modules.py:267-275) against the target's word durations
            const long long w = p.ph2word[e];
            const bool inw = w >= 1 && w < (long long)p.n_words;
            const float pr = clamp0(x), pd = w > 0 ? pr : pr * 0.f;
            float alpha = 0.f;
            if (inw) {
                const size_t o = (size_t)b * W1 + (size_t)(w - 1);
                const float win = p.wdur_pred[o];
                alpha = p.wdur_gt[o] / (win < 1e-5f ? 1e-5f : win);
            }
            const float align = rintf(pd * alpha);
            const bool valid = !p.mask || p.mask[e];
            a.i[2] += (valid && fabsf(align - y) <= y * p.tol_pdur) ? 1 : 0;
            a.i[3] += valid ? 1 : 0;
        } else if (e < nph + nwd) {
            const unsigned j = e - nph, b = j / W1;
            const long long w = (long long)(j - b * W1) + 1;
            const float wp = p.wdur_pred[j], wg = p.wdur_gt[j];
            a.d[1] += dur_term(wp, wg, p.offset, p.kind);
            bool valid = true;
            if (p.mask) {                                       // duration.py:51-53: any phoneme of the word is valid
                valid = false;
                const size_t row = (size_t)b * p.L;
                for (int l = 0; l < p.L; ++l) valid = valid || (p.ph2word[row + l] == w && p.mask[row + l]);
            }
            a.i[0] += (valid && fabsf(wp - wg) <= wg * p.tol_rhythm) ? 1 : 0;
            a.i[1] += valid ? 1 : 0;
        } else {
            const size_t row = (size_t)(e - nph - nwd) * p.L;
            float sp = 0.f, sg = 0.f;
            for (int l = 0; l < p.L; ++l) {
                sp += clamp0(p.dur_pred[row + l]);
                sg += p.dur_gt[row + l];
            }
            a.d[2] += dur_term(sp, sg, p.offset, p.kind);
        }
    });
}

struct FinalP {
    void* out;
    double den[3];      // what each double sum is divided by for its mean
};
enum { FINAL_LOSS, FINAL_CURVE, FINAL_DUR };

// thread i adds the partials i, i + 256, ... of a slot, then the workgroup's fixed-order sum
template <int KIND>
__global__ __launch_bounds__(kScoreThreads) void score_final_kernel(const void* ws, int nblocks, const FinalP f) {
    __shared__ double shd[kScoreThreads];
    __shared__ long long shi[kScoreThreads];
    const double* wd = static_cast<const double*>(ws);
    const long long* wi = static_cast<const long long*>(ws);
    double d[kAccD];
    long long n[kAccI];
    for (int j = 0; j < kAccD; ++j) {
        double s = 0.0;
        for (int k = threadIdx.x; k < nblocks; k += kScoreThreads) s += wd[j * kScoreMaxBlocks + k];
        d[j] = block_sum(s, shd);
    }
    for (int j = 0; j < kAccI; ++j) {
        long long s = 0;
        for (int k = threadIdx.x; k < nblocks; k += kScoreThreads) s += wi[(kAccD + j) * kScoreMaxBlocks + k];
        n[j] = block_sum(s, shi);
    }
    if (threadIdx.x != 0) return;
    if (KIND == FINAL_LOSS) {
        double* out = static_cast<double*>(f.out);
        out[0] = d[0];
        out[1] = d[0] / f.den[0];
    } else if (KIND == FINAL_CURVE) {
        dsd_curve_result* out = static_cast<dsd_curve_result*>(f.out);
        out->close = n[0];
        out->total = n[1];
        out->sum_target = d[0];
        out->sum_target_sq = d[1];
        out->sum_residual_sq = d[2];
    } else {
        dsd_dur_result* out = static_cast<dsd_dur_result*>(f.out);
        out->pdur_sum = d[0];
        out->wdur_sum = d[1];
        out->sdur_sum = d[2];
        out->pdur_mean = d[0] / f.den[0];
        out->wdur_mean = d[1] / f.den[1];
        out->sdur_mean = d[2] / f.den[2];
        out->rhythm_correct = n[0];
        out->rhythm_total = n[1];
        out->pdur_accurate = n[2];
        out->pdur_total = n[3];
    }
}

}  // namespace

hipError_t launch_diffuse(const DiffuseP& p, int items, hipStream_t st) {
    const unsigned threads = (unsigned)(((p.cols + 3) >> 2) * (long)p.rows);
    const dim3 grid((threads + 255u) / 256u, items);
    const uintptr_t ptrs = (uintptr_t)p.x_t | (uintptr_t)p.target | (uintptr_t)p.x0 | (uintptr_t)p.eps;
    if (p.cols % 4 == 0 && (ptrs & 15) == 0) diffuse_kernel<true><<<grid, 256, 0, st>>>(p);
    else diffuse_kernel<false><<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}

hipError_t launch_masked_loss(const LossP& p, void* ws, double* out, hipStream_t st) {
    const long long n = (long long)p.B * p.rows * p.cols;
    const int blocks = score_blocks(n);
    loss_kernel<<<blocks, kScoreThreads, 0, st>>>(p, (unsigned)n, ws);
    FinalP f;
    f.out = out;
    f.den[0] = (double)n;
    f.den[1] = f.den[2] = 1.0;
    score_final_kernel<FINAL_LOSS><<<1, kScoreThreads, 0, st>>>(ws, blocks, f);
    return hipGetLastError();
}

hipError_t launch_curve_stats(const float* pred, const float* target, const unsigned char* mask, long long n, float tol, void* ws,
                              void* out, hipStream_t st) {
    const int blocks = score_blocks(n);
    curve_kernel<<<blocks, kScoreThreads, 0, st>>>(pred, target, mask, (unsigned)n, tol, ws);
    FinalP f;
    f.out = out;
    f.den[0] = f.den[1] = f.den[2] = 1.0;
    score_final_kernel<FINAL_CURVE><<<1, kScoreThreads, 0, st>>>(ws, blocks, f);
    return hipGetLastError();
}

hipError_t launch_dur_score(const DurP& p, void* ws, void* out, hipStream_t st) {
    const long long nph = (long long)p.B * p.L, nwd = (long long)p.B * (p.n_words - 1), n = nph + nwd + p.B;
    const long long words = (long long)p.B * p.n_words;
    dur_words_kernel<<<(unsigned)((words + kScoreThreads - 1) / kScoreThreads), kScoreThreads, 0, st>>>(p);
    const int blocks = score_blocks(n);
    dur_terms_kernel<<<blocks, kScoreThreads, 0, st>>>(p, (unsigned)n, ws);
    FinalP f;
    f.out = out;
    f.den[0] = (double)nph;
    f.den[1] = (double)nwd;
    f.den[2] = (double)p.B;
    score_final_kernel<FINAL_DUR><<<1, kScoreThreads, 0, st>>>(ws, blocks, f);
    return hipGetLastError();
}

}  // namespace dsd
