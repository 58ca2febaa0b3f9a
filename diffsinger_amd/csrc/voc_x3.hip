// NSF-HiFiGAN residual-block convolution in SPLIT-bf16 arithmetic ("bf16x3"; opt-in: dsd_set_precision on a vocoder handle).
//
// A k-tap dilated Conv1d(C -> C) of a ResBlock1 / ResBlock2 (models.py:62-69, 92-97):
//   out[o][t] = lrelu_out( bias[o] + sum_{tap, c} W[o][c][tap] * lrelu_in(x)[c][t + (tap - k/2) dil] ) (+ res[o][t])
// with the arithmetic contract of wn_layer_x3.hip: every operand of the product is split x = hi + lo, hi = bf16(x),
// lo = bf16(x - hi) (round to nearest even), the product is lo.hi + hi.lo + hi.hi on v_mfma_f32_16x16x32_bf16 with fp32
// accumulators.  The leaky ReLU on the input is applied in fp32 BEFORE the split (slope 1: none); bias, the output's leaky ReLU
// (slope 1: none) and the residual add are fp32 in the epilogue; every buffer is fp32; frames outside [0, item length) are zero
// padding.
//
// Tile: one workgroup of 4 waves = all C output rows x BN = 16 NCB frames (32 or 64).  Wave w owns the 16 MBW rows
// [16 MBW w, 16 MBW (w + 1)), MBW = ceil(C / 64) - rows at or above C are zero rows of the weight stream and are not stored
// (C = 96 / 160 / 224 waste a quarter to a twelfth of the MFMAs; C a multiple of 64 none).
//   * weights pre-split at finalize and packed in the order a wave consumes them, [wave][k32 step = tap * C/32 + chunk]
//     [row block][hi | lo][lane][8 bf16] (api.hip, pack_voc_x3): one linear stream of 1 KiB blocks per wave, through a ring of
//     three k32 steps in registers, each refill issued right behind the MFMAs that free its slot and pinned there;
//   * the activation tile (BN + 2 HL frames, HL = the reach (k/2) dil rounded up to 4) staged transposed as two bf16 images
//     [frame][channel] with rows of 2 C + 16 bytes - (C/2 + 4) / 4 is odd, so the 16 frames of a fragment read fall on 64
//     distinct banks - a tap is a row shift and a B fragment one ds_read_b128 per image at any dilation;
//   * the hi / lo split is formed from the global loads in the staging pass;
//   * the K walk (taps outermost, 32-channel chunks inside, hi/lo order inside a step) is the packed stream's and the same for
//     every tile width and for ragged and dense launches: an output value does not depend on how the frames were tiled.
// LDS: 4 (BN + 2 HL)(C + 8) bytes.  C = 256: 64 frames + 2 x 28 = 127 KB fits, 64 + 2 x 48 = 169 KB does not - the host takes
// 32-frame tiles there (135 KB).  C <= 256 is the bound of this file: C = 512 would need MBW = 8 (fits in registers) but only
// reaches HL <= 20 at 32 frames, and no generator layout has a 512-channel residual stage.
// Addressing: lane offsets are 32-bit, so the host admits a launch only while C * Ts * 4 bytes stay below 2^31.
#include <hip/hip_ext.h>

#include "dsd_internal.h"
#include "dsd_device.h"

namespace dsd {
constexpr int kGroup = KG_VOCODER;      // whose create functions prepare this file's kernels (dsd_internal.h: KernelReg)

// MBW: 16-row blocks per wave; NCB: 16-frame column blocks per tile; RAG: ragged batch (the valid (item, tile) list)
template <int MBW, int NCB, int RAG>
__global__ __launch_bounds__(256, 1) void voc_conv_x3_kernel(const VocX3P p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int BN = 16 * NCB;
    constexpr int ES = BN + 4;                           // epilogue tile row stride (floats)
    constexpr int RD = 3;                                // weight ring: k32 steps in registers (MBW x (hi + lo) x 4 VGPRs each)
    const int C = p.C, RS = C + 8, HL = p.HL, Ts = p.Ts;
    const int NF = BN + 2 * HL;                          // staged frames
    __bf16* xhi = reinterpret_cast<__bf16*>(lds_raw);    // [NF][RS]
    __bf16* xlo = xhi + NF * RS;                         // [NF][RS]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane >> 4, lcol = lane & 15, rq = lrow * 4;
    const int work = xcd_work();
    const int rest = RAG ? p.cgmap[work] : work;
    const int b = fdiv_floor(rest, p.inv_tiles_per_b);
    const int t0 = (rest - b * p.tiles_per_b) * BN;
    const int Tb = (RAG && p.lens) ? p.lens[b] : p.T;
    const int bu = __builtin_amdgcn_readfirstlane(b), t0u = __builtin_amdgcn_readfirstlane(t0);

    // this wave's weight stream; the first RD steps go out before the staging pass
    const int nsteps = p.nsteps;
    const __amdgpu_buffer_rsrc_t r_w = rsrc(reinterpret_cast<const unsigned char*>(p.W) + (long)wave * nsteps * (MBW * 2048));
    bf16x8 Wh[RD][MBW], Wl[RD][MBW];
    auto w_issue = [&](auto J, int s) {                  // step s -> ring slot J
#pragma unroll
        for (int k = 0; k < MBW; ++k) {
            Wh[J][k] = ldw(r_w, lane * 16, (s * MBW + k) * 2048);
            Wl[J][k] = ldw(r_w, lane * 16, (s * MBW + k) * 2048 + 1024);
        }
    };
    static_for<0, RD>([&](auto J) {
        if (J < nsteps) w_issue(J, J);
    });

    // ---------------- staging: leaky ReLU, zero padding, split hi / lo, transpose to [frame][channel] ----------------
    {
        const __amdgpu_buffer_rsrc_t r_x = rsrc(p.x + (long)bu * p.bstride + (t0u - HL));      // inside the arena's guard at t0 = 0
        const int nunit = (C >> 3) * p.nfq;              // units of 8 channels x 4 frames
        const float slope = p.slope_in;
        for (int u = tid; u < nunit; u += 256) {
            const int co = fdiv_floor(u, p.inv_nfq), fq = u - co * p.nfq;       // channel octet, frame quad
            f32x4 sv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) sv[c] = ld4(r_x, ((8 * co + c) * Ts + 4 * fq) * 4, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int fr = 4 * fq + e;
                const int t = t0 - HL + fr;
                const bool ok = t >= 0 && t < Tb;
                bf16x8 h8, l8;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    float v = ok ? sv[c][e] : 0.f;
                    v = v >= 0.f ? v : v * slope;
                    const __bf16 hv = (__bf16)v;
                    h8[c] = hv;
                    l8[c] = (__bf16)(v - (float)hv);
                }
                *reinterpret_cast<bf16x8*>(&xhi[fr * RS + 8 * co]) = h8;
                *reinterpret_cast<bf16x8*>(&xlo[fr * RS + 8 * co]) = l8;
            }
        }
    }
    __syncthreads();

    // ---------------- K walk: k32 step = [tap][32-channel chunk] ----------------
    f32x4 acc[MBW][NCB];
#pragma unroll
    for (int k = 0; k < MBW; ++k)
#pragma unroll
        for (int n = 0; n < NCB; ++n) acc[k][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B fragment of a step: lane (g = lrow, column lcol) holds channels 32 chunk + 8 g .. + 7 of frame HL + 16 n + lcol + (tap - k/2) dil
    const int nch = C >> 5;
    const int tap_step = p.dil * RS - 32 * nch;          // from the last chunk of a tap to the first of the next
    int boff = (HL + lcol - (p.taps >> 1) * p.dil) * RS + 8 * lrow;
    int chunk = 0;
    for (int s0 = 0; s0 < nsteps; s0 += RD) {
        static_for<0, RD>([&](auto J) {
            const int s = s0 + J;
            if (s < nsteps) {
                bf16x8 bh[NCB], bl[NCB];
#pragma unroll
                for (int n = 0; n < NCB; ++n) {
                    bh[n] = *reinterpret_cast<const bf16x8*>(&xhi[boff + 16 * n * RS]);
                    bl[n] = *reinterpret_cast<const bf16x8*>(&xlo[boff + 16 * n * RS]);
                }
#pragma unroll
                for (int k = 0; k < MBW; ++k) x3_products<NCB>(acc[k], Wh[J][k], Wl[J][k], bh, bl);
                if (s + RD < nsteps) w_issue(J, s + RD); // the slot is free again
                boff += 32;
                if (++chunk == nch) {
                    chunk = 0;
                    boff += tap_step;
                }
                // (pinned: left to itself the scheduler sinks the refill to just before its use and the ring collapses)
                __builtin_amdgcn_sched_barrier(0);
            }
        });
    }

    // ---------------- epilogue: bias, leaky ReLU, residual - fp32, row-major through the wave's LDS tile ----------------
    __syncthreads();                                     // every wave is done reading the images
    float* ew = reinterpret_cast<float*>(lds_raw) + wave * (16 * MBW * ES);      // wave-private [16 MBW][ES]
#pragma unroll
    for (int k = 0; k < MBW; ++k)
#pragma unroll
        for (int n = 0; n < NCB; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) ew[(k * 16 + rq + r) * ES + n * 16 + lcol] = acc[k][n][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        constexpr int NE = MBW * NCB;                    // float4 per lane: 16 MBW rows x BN / 4
        const int orow0 = 16 * MBW * wave;
        const long eoff = (long)bu * p.bstride + (long)orow0 * Ts + t0u;
        const bool has_res = p.res != nullptr;
        const __amdgpu_buffer_rsrc_t r_b = rsrc(p.bias + orow0);
        const __amdgpu_buffer_rsrc_t r_e = rsrc((has_res ? p.res : p.x) + eoff);
        const dsd_i32x4 w_o = dsd_rsrc_words(p.out + eoff);
        const float so = p.slope_out;
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            const int idx = lane + 64 * m;
            const int rowl = idx / (BN / 4), c4 = idx % (BN / 4);
            if (orow0 + rowl < C) {
                const int voff = (rowl * Ts + 4 * c4) * 4;
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&ew[rowl * ES + 4 * c4]);
                const float bv = ld1(r_b, rowl * 4, 0);
                f32x4 rv = f32x4{0.f, 0.f, 0.f, 0.f};
                if (has_res) rv = ld4(r_e, voff, 0);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = a4[e] + bv;
                    o[e] = (v >= 0.f ? v : v * so) + rv[e];
                }
                st4_l2(o, w_o, voff, 0);
            }
        }
    }
}

int voc_x3_mbw(int C) { return (C + 63) / 64; }

int voc_x3_lds_bytes(int C, int hl, int ncb) {
    const int img = 4 * (16 * ncb + 2 * hl) * (C + 8), epi = 4 * 16 * voc_x3_mbw(C) * (16 * ncb + 4) * 4;
    return img > epi ? img : epi;
}

// the widest tile (column blocks) whose images fit, 0: none - the convolution stays on the fp32 kernel
int voc_x3_max_ncb(int C, int taps, int dil) {
    if (C < 64 || C > 256 || C % 32 != 0 || taps < 1 || taps % 2 == 0 || dil < 1) return 0;
    const int hl = round_up((taps / 2) * dil, 4);
    if (hl > 64) return 0;                               // the arena's guard covers the halo over-reads of the first / last tile
    for (int ncb : {4, 2})
        if (voc_x3_lds_bytes(C, hl, ncb) <= kMaxDynLds) return ncb;
    return 0;
}

template <int MBW, int NCB, int RAG>
static hipError_t voc_x3_launch(const VocX3P& p, int ntiles, hipStream_t st) {
    if (ntiles == 0) return hipSuccess;          // a ragged batch of empty items
    return launch_timed<voc_conv_x3_kernel<MBW, NCB, RAG>, kGroup>(dim3(ntiles), dim3(256), voc_x3_lds_bytes(p.C, p.HL, NCB), st, p,
                                                                   "voc_conv_x3_kernel<%d, %d, %d>", MBW, NCB, RAG);
}

template <int MBW>
static hipError_t voc_x3_pick(const VocX3P& p, int ncb, int ntiles, hipStream_t st) {
    if (ncb == 4) return p.cgmap ? voc_x3_launch<MBW, 4, 1>(p, ntiles, st) : voc_x3_launch<MBW, 4, 0>(p, ntiles, st);
    return p.cgmap ? voc_x3_launch<MBW, 2, 1>(p, ntiles, st) : voc_x3_launch<MBW, 2, 0>(p, ntiles, st);
}

// ncb: 2 = 32-frame tiles, 4 = 64-frame tiles; ntiles: workgroups (ragged: p.ncg)
hipError_t launch_voc_x3(const VocX3P& p, int ncb, int ntiles, hipStream_t st) {
    if ((ncb != 2 && ncb != 4) || voc_x3_max_ncb(p.C, p.taps, p.dil) < ncb) return hipErrorInvalidValue;
    switch (voc_x3_mbw(p.C)) {
        case 1: return voc_x3_pick<1>(p, ncb, ntiles, st);
        case 2: return voc_x3_pick<2>(p, ncb, ntiles, st);
        case 3: return voc_x3_pick<3>(p, ncb, ntiles, st);
        case 4: return voc_x3_pick<4>(p, ncb, ntiles, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace dsd
