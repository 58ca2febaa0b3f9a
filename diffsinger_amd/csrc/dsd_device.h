// Device primitives shared by the hand-written kernel files of libdsdenoise (gfx950, device code only; included after
// dsd_internal.h): vector types, buffer-descriptor loads and the 16-byte store with its two cache policies, index helpers,
// the compensated DFT tile walk, the activations named for their arithmetic, the split-bf16 products, the counter-based random draws and the diagnostic stamps.
#pragma once
#include <type_traits>

#include "dsd_internal.h"

namespace dsd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned dsd_u32x4 __attribute__((ext_vector_type(4)));
typedef int dsd_i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// Buffer descriptors.  Every global access of the layer kernels goes through one built from wave-uniform values: 32-bit lane
// offsets + SGPR offsets + immediates, no 64-bit address arithmetic.
// ---------------------------------------------------------------------------------------------
constexpr unsigned kRange = 0x7FFFFFF0u;
constexpr int kRsrcFlags = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* ptr) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, kRange, kRsrcFlags);
}
__device__ __forceinline__ f32x4 ld4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ bf16x8 ldw(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ float ld1(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// 16-byte raw buffer store followed by two wait states, as ONE inline-asm statement.  A store of more than 8 bytes reads its
// data registers over several cycles after issue, and a VALU write to one of them in the next issue slot can land first.
// hipcc (ROCm 7.2) inserts the required wait state for the immediate-soffset form but not when soffset is a register - LLVM's
// hazard model calls that form safe - and on gfx950 it is not: wn_out_rw_kernel<4, *> stored, nondeterministically and in
// ~0.4 % of the elements, the NEXT item's operand as the first element of a vector (found with tools/harness/
// rows_harness.hip; tools/check_store_hazard.py scans the ISA of every kernel file for the pattern, tests/
// test_kernel_resources.py runs it).  A separate `s_nop` (builtin or asm) behind the builtin store does not stay there -
// neither scheduling barriers nor a memory clobber kept the post-RA scheduler from moving VALU instructions in between -
// so the store itself is asm.  `rsrc` = the four descriptor words (dsd_rsrc_words), wave-uniform.
__device__ __forceinline__ dsd_i32x4 dsd_rsrc_words(const void* ptr) {
    // (readfirstlane: the words must be in SGPRs for the asm's "s" operand - when the compiler cannot prove the pointer
    // wave-uniform, or has spilled it to a VGPR, it would otherwise print a VGPR range into the descriptor slot)
    const unsigned long long a = (unsigned long long)ptr;
    return dsd_i32x4{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu)),
                     (int)kRange, kRsrcFlags};
}
template <int AUX>
__device__ __forceinline__ void dsd_store_b128(dsd_u32x4 data, dsd_i32x4 rsrc, int voff, int soff) {
    static_assert(AUX == 0 || AUX == 16, "plain or sc1 (write-through)");
    if (AUX == 16)
        asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen sc1\n\ts_nop 1" ::"v"(data), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    else
        asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" ::"v"(data), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}

// Cache policy of the 16-byte result stores (bit 4 = sc1 = write-through).
// st4_wt - write-through: the WaveNet layer kernels' x / skip and the edge kernel's outputs.  A kernel boundary costs the bytes
// its predecessor left dirty in the L2s / ~6 TB/s (MI355X_MICROARCH.md, "boundary": x + skip of a fused layer at B = 8 are
// 16 MB); write-through stores spread that over the kernel's own epilogues.  Measured against plain stores on fresh boxes:
// 50-NFE loop 16.68 -> 16.55 ms at B = 1, 26.21 -> 25.79 at B = 2, 70.07 -> 69.00 at B = 8, the variance pair 37.54 -> 36.92.
// st4_l2 - plain: what the very next launch reads back stays in L2.  The row-split / wide-row conv's z: same-box A/B of the
// 50-NFE loop at B = 1, three runs each: x / skip write-through + z plain 16.52 ms, both write-through 16.55, x / skip plain
// + z write-through 16.70, both plain 16.67.  LYNXNet's kernels: write-through measured +0.5 %.
constexpr int kStAux = 16;
__device__ __forceinline__ void st4_wt(f32x4 v, dsd_i32x4 r, int voff, int soff) {
    dsd_store_b128<kStAux>(__builtin_bit_cast(dsd_u32x4, v), r, voff, soff);
}
__device__ __forceinline__ void st4_l2(f32x4 v, dsd_i32x4 r, int voff, int soff) {
    dsd_store_b128<0>(__builtin_bit_cast(dsd_u32x4, v), r, voff, soff);
}

// ---------------------------------------------------------------------------------------------
// Index arithmetic and scheduling
// ---------------------------------------------------------------------------------------------
// floor(x / d) for 0 <= x < 2^22 with inv = 1.0f / d: one cvt + mul + cvt instead of the ~40-instruction
// integer-division expansion (the kernel prologue is on the latency-critical path at B = 1)
__device__ __forceinline__ int fdiv_floor(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }

// byte offset of a row as a 24-bit multiply (rows < 512; the host keeps Ts below 2^22): a 32-bit `row * Ts + c` compiles to
// v_mad_u64_u32, whose 64-bit addend has an undefined high half - the register allocator parked it on a register with a load
// in flight (the FiLM value) and the hardware dependency put an s_waitcnt vmcnt(0) in front of the x-tile loads.
__device__ __forceinline__ int row_ts(int row, int Ts) { return (int)__umul24((unsigned)row, (unsigned)(Ts * 4)); }   // BYTES

// XCD-aware bijective remap of a 1-D grid (speed only, any grid size): the dispatcher deals workgroups round-robin over the
// 8 XCDs, so blocks b and b + 8 share an L2; XCD k takes a CONTIGUOUS range of the returned work items instead, so
// neighbouring items - the row tiles of one frame tile, which stage the same activations, or frame tiles that share halo
// columns - share an L2.
__device__ __forceinline__ int xcd_work() {
    const int nwg = gridDim.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// a walk's steps with their index a constant expression (ring slots, the block each step issues)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Every field of a WaveNet layer's argument block in SGPRs behind ONE batch of scalar loads at the top of the kernel: left to
// itself the compiler fetches them in two or three dependent batches (each a cold scalar-cache round trip) before the first
// vector load can issue - on kernels whose whole life is 8-20 k cycles.  (The unpinned form was measured against this and removed.)
__device__ __forceinline__ void wn_pin_args(const WnLayerP& p) {
    asm volatile("" ::"s"(p.Aconv), "s"(p.Aout), "s"(p.bias_out), "s"(p.xin), "s"(p.xout), "s"(p.skip), "s"(p.z), "s"(p.x_bstride),
                 "s"(p.Ts), "s"(p.cp), "s"(p.cp_bstride), "s"(p.film), "s"(p.film_cstride), "s"(p.film_col0), "s"(p.film_colb),
                 "s"(p.dil), "s"(p.T), "s"(p.tiles_per_b), "s"(p.first_layer), "s"(p.inv_tiles_per_b), "s"(p.tile0),
                 "s"((int)gridDim.x));                           // (the grid size is an implicit argument: same segment)
}

__device__ __forceinline__ f32x4 mfma_16x16x4(float wfrag, float xfrag, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(wfrag, xfrag, acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// The compensated DFT tile walk of mel_dft_kernel and hs_dft_kernel: [kDftRows basis rows] x [kDftFrames frames] per
// workgroup of 256, wave w owns basis rows 16w..16w+15 and all 64 frames (four 16x16 accumulators).  Operand maps of
// v_mfma_f32_16x16x4_f32: A[i = lane & 15][k = lane >> 4] (basis rows), B[k = lane >> 4][j = lane & 15] (frames);
// D[row = 4 (lane >> 4) + reg][col = lane & 15].
// Accuracy: one fp32 accumulator over all K taps carries the rounding of large partial sums that
// cancel by the end, so each kDftKS taps go into a fresh accumulator (2 MFMAs) and the partial sums are added with TwoSum
// into a (hi, lo) pair; the caller's epilogue reads hi + lo.
// bas = the row tile of a basis [.][Kpad] (K <= Kpad, a multiple of kDftTaps); stage(f, j) = the B operand of frame f < nf,
// tap j < K of the tile (zero elsewhere); sA / sB = LDS of kDftRows / kDftFrames rows of kDftLS floats.
// ---------------------------------------------------------------------------------------------
constexpr int kDftKS = 8;               // taps per fresh MFMA accumulator
constexpr int kDftLS = kDftTaps + 4;    // LDS row stride: the 16 rows x 4 taps of an MFMA operand read hit 64 distinct banks
template <typename Stage>
__device__ __forceinline__ void dft_tile_walk(const float* __restrict__ bas, int Kpad, int K, int nf, float* sA, float* sB,
                                              Stage&& stage, f32x4 (&hi)[4], f32x4 (&lo)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int f = 0; f < 4; ++f) hi[f] = lo[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += kDftTaps) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < (kDftRows * kDftTaps) / 256; ++s) {
            const int idx = tid + 256 * s, row = idx / kDftTaps, kk = idx % kDftTaps;
            sA[row * kDftLS + kk] = bas[(long)row * Kpad + k0 + kk];
        }
#pragma unroll
        for (int s = 0; s < (kDftFrames * kDftTaps) / 256; ++s) {
            const int idx = tid + 256 * s, f = idx / kDftTaps, kk = idx % kDftTaps, j = k0 + kk;
            sB[f * kDftLS + kk] = (f < nf && j < K) ? stage(f, j) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int half = 0; half < kDftTaps / kDftKS; ++half) {
            f32x4 part[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) part[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = half * kDftKS / 4; ks < (half + 1) * kDftKS / 4; ++ks) {
                const float a = sA[(16 * w + (lane & 15)) * kDftLS + 4 * ks + (lane >> 4)];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const float bv = sB[(16 * f + (lane & 15)) * kDftLS + 4 * ks + (lane >> 4)];
                    part[f] = mfma_16x16x4(a, bv, part[f]);
                }
            }
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {       // TwoSum: hi + lo carries the running sum to about 2 x 24 bits
                    const float x = part[f][r], s = hi[f][r] + x, bp = s - hi[f][r];
                    lo[f][r] += (hi[f][r] - (s - bp)) + (x - bp);
                    hi[f][r] = s;
                }
        }
    }
}

// one row block x all NCB 16-frame column blocks of a k32 step in split-bf16 arithmetic: lo.hi, hi.lo, hi.hi (smallest terms
// first), the accumulators alternating
template <int NCB>
__device__ __forceinline__ void x3_products(f32x4 (&a)[NCB], bf16x8 wh, bf16x8 wl, const bf16x8 (&bh)[NCB], const bf16x8 (&bl)[NCB]) {
#pragma unroll
    for (int n = 0; n < NCB; ++n) a[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, bh[n], a[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NCB; ++n) a[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, bl[n], a[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NCB; ++n) a[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, bh[n], a[n], 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// Activations, named for their arithmetic (the forms round differently and are not interchangeable)
// ---------------------------------------------------------------------------------------------
// WaveNet gate on the hardware exp / rcp units (v_exp_f32, v_rcp_f32: ~1 ulp each).  Absolute error of sigmoid(g) * tanh(f)
// stays below 3e-7 - far inside the 2e-5 per-evaluation parity tolerance - at a fifth of the instruction count of libm's
// expf / tanhf (the gate is ~1 k cycles of a 23 k-cycle workgroup at B = 1).
__device__ __forceinline__ float sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }
__device__ __forceinline__ float tanh_fast(float v) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * v)); }
// LYNXNet's SwiGLU in lynx_layer.hip / lynx_x3.hip: expf as the library computes it; the reciprocal as v_rcp_f32 (<= 1 ulp)
// instead of an IEEE division sequence (~10 VALU instructions per element, 64 elements per lane and row tile in the epilogue)
__device__ __forceinline__ float sigmoid_rcp(float v) { return __builtin_amdgcn_rcpf(1.f + expf(-v)); }

// ---------------------------------------------------------------------------------------------
// Counter-based random draws (noise_kernels.hip; the specification is in include/dsdenoise.h above dsd_noise_fill).
// Philox4x32-10 (Salmon et al., Random123): ten rounds of two 32 x 32 -> 64-bit products, the key bumped between rounds.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ dsd_u32x4 philox4x32_10(dsd_u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = dsd_u32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// ((w >> 9) + 0.5) * 2^-23: every step exact in fp32 (k + 0.5 with k < 2^23 needs 24 bits), strictly inside (0, 1)
__device__ __forceinline__ float philox_uniform(unsigned w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }
// Box-Muller on one word pair with the precise logf / sqrtf / sincosf: |z| <= sqrt(-2 ln 2^-24) = 5.7681
__device__ __forceinline__ void philox_normal2(unsigned w0, unsigned w1, float& z0, float& z1) {
    const float r = sqrtf(-2.f * logf(philox_uniform(w0)));
    float s, c;
    sincosf(6.283185307179586f * philox_uniform(w1), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// ---------------------------------------------------------------------------------------------
// The prefix sum of one row of at most 8 * 256 counts by a workgroup of 256 lanes (frames_kernels.hip, words_kernels.hip):
// cum[i] = min(value(0) + .. + value(i), cap) for i < n.  Each lane sums `per` contiguous values, the 256 lane totals are
// scanned through `part` (256 ints), and the lane adds what stands before it.  value(i) must lie in [0, cap]: every partial
// sum then saturates at cap, so nothing overflows, and a sum that has reached cap stays there.  Ends on a barrier: every
// lane may read all of cum afterwards.  `cum` and `part` are LDS; all 256 lanes must call.
// ---------------------------------------------------------------------------------------------
template <typename Value>
__device__ __forceinline__ void block_prefix_capped(int* cum, int* part, int n, int cap, Value&& value) {
    const int tid = threadIdx.x;
    const int per = (n + 255) / 256;                       // <= 8 contiguous values per lane
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int run = 0;
    for (int i = lo; i < hi; ++i) {
        run = (int)min((long long)run + value(i), (long long)cap);
        cum[i] = run;
    }
    part[tid] = run;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                    // inclusive scan of the 256 lane totals
        const int add = tid >= s ? part[tid - s] : 0;
        __syncthreads();
        part[tid] = (int)min((long long)part[tid] + add, (long long)cap);
        __syncthreads();
    }
    const int before = tid ? part[tid - 1] : 0;
    for (int i = lo; i < hi; ++i) cum[i] = (int)min((long long)cum[i] + before, (long long)cap);
    __syncthreads();
}
// the owner of frame p under such sums: the first i in [0, n) with cum[i] > p, or n (a zero count repeats its predecessor's
// sum and is never the first)
__device__ __forceinline__ int first_above(const int* cum, int n, int p) {
    int a = 0, z = n;
    while (a < z) {
        const int m = (a + z) >> 1;
        if (cum[m] > p) z = m;
        else a = m + 1;
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
// Diagnostic builds only (-DDSD_STAMPS; tools/stamp_*.py): thread 0 of workgroups < 4096 writes a clock into `elem` of its
// file's stamp array, between scheduling barriers that keep the stamp at its place in the schedule.  No output value depends
// on a stamp.  DSD_STAMP_AT: s_memtime (shader clock); DSD_STAMP_WITH(elem, __builtin_amdgcn_s_memrealtime): 100 MHz wall clock.
// ---------------------------------------------------------------------------------------------
#ifdef DSD_STAMPS
#define DSD_STAMP_WITH(elem, clock)                                                     \
    do {                                                                                \
        if (threadIdx.x == 0 && blockIdx.x < 4096) {                                    \
            __builtin_amdgcn_sched_barrier(0);                                          \
            (elem) = clock();                                                           \
            __builtin_amdgcn_sched_barrier(0);                                          \
        }                                                                               \
    } while (0)
#define DSD_STAMP_AT(elem) DSD_STAMP_WITH(elem, __builtin_amdgcn_s_memtime)
#endif

}  // namespace dsd
