// Internal declarations shared by the HIP translation units of libdsdenoise (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

namespace dsd {

// ---------------------------------------------------------------------------------------------
// Activation layout in HBM ("internal layout"): [batch][channel][Ts] fp32, time innermost,
// Ts = round_up(T, 64) + 32 floats (a multiple of 32 floats = 128 B that is never a multiple of
// 4 KiB, so the rows of a channel x time tile rotate over the memory channels).  Frames
// t in [T, Ts) are padding: kernels may write garbage there and every consumer masks on t < T
// when it stages a tile.  Every buffer lives in one arena with a 256-float guard in front and
// behind, so the halo over-reads of the first/last tile land in allocated memory (and are masked).
// ---------------------------------------------------------------------------------------------
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline int padded_ts(int T) { return round_up(T, 64) + 32; }

enum Stage { ST_PLAIN = 0, ST_FILM = 1, ST_LN = 2, ST_SCALE = 3, ST_LRELU = 4, ST_RELU = 5 };
enum Epi { EP_BIAS_ACT = 0, EP_GATE = 1, EP_RESSKIP = 2, EP_LINCOMB = 3, EP_SWIGLU = 4, EP_BIAS_RES = 5, EP_SCATTER = 6, EP_LYNX_NEXT = 7 };
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_MISH = 2, ACT_GELU = 3, ACT_LRELU = 4, ACT_TANH = 5, ACT_SILU = 6 };

// Path switches (tests, diagnostics): each forces a form the library's own rule also chooses (DSD_PRECISION selects an
// arithmetic mode).  Each handle keeps its own snapshot (dsd_handle::opts): every entry point of the C ABI that launches kernels
// takes a fresh one from the environment, so one process can drive either side of a switch through consecutive calls - this is
// how tests/test_gpu_fused.py puts every instantiation of the layer kernels under oracle parity - and dsd_get_stats reports
// from the snapshot of the handle's last call.  The snapshot is part of the hipGraph cache key (a captured graph is the launch
// sequence of ONE set of choices).  -1 = unset: the library's own rule.  Launchers outside api.hip get the switch they need as
// an argument.
struct PathOpts {
    int fused_layer = -1;   // DSD_FUSED_LAYER     0: never wn_layer.hip, 1: on every supported grid
    int fused16 = -1;       // DSD_FUSED16         0: never wn_layer16_kernel (16-frame tiles of the fused layer), 1: every layer on it
    int wn_plan = -1;       // DSD_WN_PLAN         0: one launch shape per layer (no mixed plans, no wide row tiles; whole-layer 16-frame
                            //                     fused tiles stay allowed), 1/unset: mixed plans (plan_denoise)
    int rowsplit = -1;      // DSD_ROWSPLIT        0: never wn_rowsplit.hip
    int rs_conv_q = -1;     // DSD_RS_CONV_Q       0 / 1: K-half / K-quarter layout of the row-split conv, 2: its Winograd form (wn_rowsplit_conv_layout)
    int rs_rows = -1;       // DSD_RS_ROWS         64 / 128 / 256: rows per workgroup of the row-split pair
    int edge = -1;          // DSD_EDGE            0: never wn_edge.hip, 1: on every grid
    int lynx_resident = -1; // DSD_LYNX_RESIDENT   0: never lynx_layer.hip, 1: on every supported grid
    int lynx_pw1p = -1;     // DSD_LYNX_PW1P       0: pw1 with one workgroup per (frame tile, row tile), g >= 1: g per frame tile
    int lynx_pw2q = -1;     // DSD_LYNX_PW2Q       0: never the 128-row pw2 of one-utterance grids (gemm.hip instead), 1: on every grid
    int precision = -1;     // DSD_PRECISION       1: split-bf16 (bf16x3) layer kernels where they exist (opt-in, own tolerance)
    int x3_wide = -1;       // DSD_X3_WIDE         0: never 64-frame tiles in the split-bf16 LYNXNet and vocoder kernels, 1: wherever they exist
};
static_assert(std::has_unique_object_representations<PathOpts>::value, "PathOpts has padding bytes (it is hashed as raw bytes)");

// Timing hook of bench.py (dsd_kernel_timing): api.hip arms the slot with a start / stop event pair before a launch it wants
// timed; the launcher that finds it armed goes through hipExtLaunchKernelGGL, which ties the two events to the dispatch
// packet itself (their elapsed time is the kernel's own begin -> end time, what a rocprofv3 kernel trace reports, not a
// bracket around the launch), records WHICH instantiation ran - kernel name + template arguments as rocprofv3 prints them,
// e.g. "wn_layer_kernel<4, 48, 0>" - and disarms it (one launch per arming).
struct TimingSlot {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool taken = false;
    char name[96] = {0};
};
TimingSlot& timing_slot();      // thread-local (api.hip)

// The dynamic-LDS limit of every kernel instantiation is raised to all of gfx950's 160 KiB per CU, once per instantiation and
// device and outside any stream capture.  A kernel form is declared where it is launched and nowhere else: launch_plain and
// launch_timed take the kernel as a template argument, and instantiating either one puts that kernel into a registry when
// the library is loaded - so whatever a code path can launch is in it, and nothing else is.  The create functions raise the
// limits of their groups' entries (prepare_kernels, api.hip); each kernel file names its group once, at its top.
constexpr int kMaxDynLds = 160 * 1024;
enum KernelGroup { KG_GEMM = 1, KG_WAVENET = 2, KG_LYNXNET = 4, KG_VOCODER = 8 };
// The launch ledger (dsd_kernel_ledger): every entry counts the launches of its instantiation through the two helpers, on the
// host, whether the launch executes at once or is recorded into a stream capture (a graph replay counts nothing: no helper
// runs).  One relaxed increment per launch; tests/test_gpu_kernel_ledger.py reads which instantiations a call ran.
typedef unsigned long long LaunchCount;
LaunchCount* register_kernel(const void* host_stub, int group);            // api.hip; the entry's launch counter (never null)
int kernel_registry_get(int i, const void** host_stub, int* group);        // entry i, or 0 past the last (tests/test_kernel_registry.py)
int prepare_kernels(const char* who, int device, int groups);              // DSD_OK or DSD_EHIP through fail()
template <auto kern, int GROUP>
struct KernelReg {
    static inline LaunchCount* const launches = register_kernel(reinterpret_cast<const void*>(kern), GROUP);
    static void count() { __atomic_fetch_add(launches, 1ull, __ATOMIC_RELAXED); }     // (odr-use: the registration runs at load time, not here)
};

template <auto kern, int GROUP, typename... Args>
inline hipError_t launch_plain(dim3 grid, dim3 block, int lds, hipStream_t st, const Args&... args) {
    KernelReg<kern, GROUP>::count();
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    return hipGetLastError();
}

template <auto kern, int GROUP, typename P, typename... NameArgs>
inline hipError_t launch_timed(dim3 grid, dim3 block, int lds, hipStream_t st, const P& p, const char* name_fmt,
                               NameArgs... name_args) {
    TimingSlot& ts = timing_slot();
    if (ts.e0 && ts.e1 && !ts.taken) {
        KernelReg<kern, GROUP>::count();
        hipExtLaunchKernelGGL(kern, grid, block, lds, st, ts.e0, ts.e1, 0, p);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wformat-security"
        snprintf(ts.name, sizeof(ts.name), name_fmt, name_args...);      // (every caller passes a literal)
#pragma clang diagnostic pop
        ts.taken = true;
        return hipGetLastError();
    }
    return launch_plain<kern, GROUP>(grid, block, lds, st, p);
}

constexpr int kMaxTerms = 8;
constexpr int kMaxOut = 3;

struct LinTerm {
    const float* ptr;   // nullptr: the model output of this launch
    long bstride;       // floats between batch items
    int rstride;        // floats between channel rows
    int ext;            // 1: caller tensor with row stride T (mask reads on t < T)
    float coef;
    int pad_;
};
struct LinOut {
    float* dst;         // internal layout
    int nterms;
    int pad_;
    LinTerm t[kMaxTerms];
};

// One GEMM-shaped launch:  out[m, t] = epilogue( sum_{tap, c} A[m, tap, c] * stage(B)[c, t + (tap-1)*dil] )
struct GemmP {
    // A: weights pre-packed in MFMA 16x16x4 fragment order, [mblk][64-ch chunk][tap][k16 in chunk][lane][4]
    const float* A;
    const float* bias;      // original row indexing, may be nullptr
    int M;                  // real output rows (original indexing)
    int C;                  // EP_GATE / EP_SWIGLU: rows per half; EP_RESSKIP: residual rows
    // B: activations, internal layout
    const float* B;
    long b_bstride;
    int b_rstride;
    int K;                  // input channels padded to a multiple of 16
    int Kreal;
    int KC;                 // channels staged in LDS per chunk (multiple of 16)
    int T;                  // valid frames
    int tiles_per_b;
    int mtiles;             // 64-row tiles (EP_GATE / EP_SWIGLU: 32 pairs each)
    int lds_bytes;          // dynamic LDS of this launch
    float inv_mtiles, inv_tiles_per_b, inv_w4;   // reciprocals for the prologue's index arithmetic
    // L2 blocking of the work order (many row tiles: LYNXNet's 1x1 GEMMs): row tiles are taken in groups of 2^gm_shift, a
    // group walks ALL frame tiles before the next group starts - so the ~100 workgroups an XCD runs at a time share one
    // group's weights (which stay in its 4 MiB L2) and each activation tile is fetched once per group.  0: row tile fastest
    // over all row tiles (every frame tile re-streams the whole weight matrix through L2).
    int gm_shift;
    int per_group;          // frame tiles of the launch << gm_shift
    float inv_per_group;
    int lpr_shift;          // staging: 2^lpr_shift lanes per staged row (>= float4 per row)
    int dil;                // dilation (taps > 1)
    int taps;               // kernel size along time (1, 3, or any odd k on the generic path)
    int HL;                 // halo columns staged on each side (multiple of 4, >= (taps / 2) * dil)
    int S;                  // LDS row stride in floats, S % 32 == 16
    float in_scale;         // ST_SCALE: staged value DIVIDED by this;  ST_LRELU: negative slope of the leaky ReLU
    // ST_RELU: y = max(x, 0) (the folded skip rows of the WaveNet, build_packed; unlike ST_LRELU it has the resident variants)
    // ST_FILM: y = x + film[c * film_cstride + film_col0 + b * film_colb]
    const float* film;
    int film_cstride, film_col0, film_colb;
    // ST_LN: y = (x - mean[b, t]) * rstd[b, t]; stats laid out [b][2][ln_ts]
    const float* ln_stats;
    int ln_ts;
    // epilogue
    int act;
    float* out;             // EP_BIAS_ACT / EP_GATE / EP_SWIGLU / EP_BIAS_RES destination
    long o_bstride;
    int o_rstride;
    const float* aux;       // EP_GATE: hoisted conditioner projection (+ biases); EP_BIAS_RES: residual
    long aux_bstride;
    int aux_rstride;
    float* x;               // EP_RESSKIP: residual stream, updated in place
    float* skip;            // EP_RESSKIP: running skip sum
    int first_layer;        // EP_RESSKIP: 1 = skip is written, not accumulated
    int up;                 // EP_SCATTER: upsampling factor u; row r*C + o, column t -> out[o][u*t + r] (C = p.C)
    // EP_LYNX_NEXT (LYNXNet layer transition): v = act(acc + bias) (+ aux);  with the NEXT layer's conditioner
    // projection cpn and step projection (film fields):  strong: x = v + cpn, xin = x + d;  else: x = v, xin = v + cpn + d;
    // cpn == nullptr (after the last layer): x = xin = v.  out = x, out2 = xin (may be nullptr), and per 64-row tile the
    // LayerNorm partials of xin over its rows: lnpart[b][mtile][0][t] = mean, [1][t] = sum of squared deviations.
    // ragged batches: item b is valid on [0, lens[b]) and zero-padded beyond, as if it were run alone at T = lens[b]
    // (nullptr: every item is valid on [0, T))
    const int* lens;
    // ragged batches, continued: the launch covers only the column groups (item b, frame tile ft) that hold valid frames;
    // cgmap[i] = b * tiles_per_b + ft of the i-th of them, ncg their number (nullptr: all batch * tiles_per_b of them)
    const int* cgmap;
    int ncg;
    float* out2;
    const float* cpn;
    long cpn_bstride;
    int cpn_rstride;
    int strong;
    float* lnpart;
    int lnpart_ts;
    // ... over the first ln_rows of the M rows only: a network run with zero-padded channels (api.hip, pad_weights) takes its
    // LayerNorm over the real ones, so tile i holds n_i = clamp(ln_rows - 64 i, 0, 64) rows for the statistics (M: all of them)
    int ln_rows;
    int nout;               // EP_LINCOMB
    LinOut lo[kMaxOut];
};

// gemm.hip
hipError_t launch_gemm(const GemmP& p, int stage, int taps, int epi, int nb, int fast, int batch, hipStream_t st);
bool gemm_has_fast(int taps, int nb, int S);
int gemm_lds_bytes(int KC, int S);
int gemm_lds_bytes_fast(int S, int stage, int taps, int K, int nb, int resident);
int gemm_fast_chunk_rows(int taps, int nb);

// wn_layer.hip: one WaveNet residual layer (conv + FiLM + gate + out-proj + residual / skip) per launch, for grids of
// at least one 32-frame tile per CU
struct WnLayerP {
    const float* Aconv;     // packed dilated-conv weights (PackedGemm, pairC = C): [2C/16 blocks][C/64 * 12 k16][64][4]
    const float* Aout;      // packed output-projection weights: [2C/16 blocks][C/16 k16][64][4]
    const float* bias_out;  // output-projection bias [2C]
    const float* xin;       // residual stream, internal layout [B][C][Ts]: read (tile + halo)
    float* xout;            // residual stream after the layer (a different buffer: neighbours read xin's halo)
    float* skip;            // running skip sum, updated in place
    float* z;               // row-split pair only (wn_rowsplit.hip): the gated conv output between the two launches
    long x_bstride;         // floats between batch items of x / skip / z
    int Ts;
    const float* cp;        // this layer's hoisted conditioner projection rows [2C][Ts] (+ conv bias + its own bias)
    long cp_bstride;
    const float* film;      // step table: d[c] = film[c * film_cstride + film_col0 + b * film_colb]
    int film_cstride, film_col0, film_colb;
    int dil, T, tiles_per_b, first_layer;
    float inv_tiles_per_b;
    const int* lens;        // ragged batches: per-item valid length (nullptr: T)
    const int* cgmap;       // ragged batches: the (item, 32-frame tile) column groups that hold valid frames
    int ncg;
    int tile0;              // dense batches: the launch covers tiles [tile0, tile0 + ntiles) of the batch's (item, frame tile)
                            // order - a layer may run as several launches over disjoint tile ranges (api.hip, wn_plan_for)
    int ntiles;             // ... their number (0: all of batch * tiles_per_b; ragged: ncg)
};
hipError_t launch_wn_layer(const WnLayerP& p, int C, int batch, hipStream_t st, int bn = 32);      // bn: 32, or 16 (wn_layer16_kernel)
bool wn_layer16_supported(int C, int dil);
bool wn_layer_supported(int C, int dil);
// wn_rowsplit.hip: the same layer as two launches with the 2C rows split over 2C / 64 workgroups per 32-frame tile, for
// grids too small for full-row tiles.  which = 0: conv + FiLM + gate (xin -> z); 1: out-proj + residual / skip (in place
// when xout == xin).  layout = wn_rowsplit_conv_layout(p, batch, bn, DSD_RS_CONV_Q): 0 / 1 the direct K-half / K-quarter conv, 2 the
// K-quarter conv on Winograd F(2,3) operands - p.Aconv stays the layer's direct packed matrix, the kernel forms G1, G2 from its taps
int wn_rowsplit_conv_layout(const WnLayerP& p, int batch, int bn, int conv_q);
hipError_t launch_wn_rowsplit(const WnLayerP& p, int which, int C, int batch, int bn, int layout, hipStream_t st);
bool wn_rowsplit_supported(int C, int dil, long Ts);

// wn_layer_x3.hip: the fused layer in split-bf16 arithmetic (opt-in precision mode); p.Aconv / p.Aout = the layer's bf16x3
// weight streams [wave][k32 step][row block][hi | lo][lane][8 bf16]
hipError_t launch_wn_layer_x3(const WnLayerP& p, int C, int batch, hipStream_t st);
bool wn_layer_x3_supported(int C, int dil);

// wn_rows.hip: the same two launches with 128 or 256 rows per workgroup (4 / 2 workgroups per 32-frame tile), for grids between
// the one-utterance case and one tile per CU
hipError_t launch_wn_rows(const WnLayerP& p, int which, int C, int batch, int rows, hipStream_t st);
bool wn_rows_supported(int C, int dil, long Ts);

// wn_edge.hip: the WaveNet's small GEMMs around the residual layers (skip projection -> output projection + solver update ->
// the next evaluation's input projection) as one launch with one workgroup per frame tile
constexpr int kEdgeMaxTerms = 8;      // state-buffer / noise terms of all outputs of one evaluation together
struct EdgeTerm {
    const float* ptr;       // state buffer (internal layout)
    long bstride;
    int rstride, ext;
    float coef;
    int out;                // the output this term belongs to
};
struct WnEdgeP {
    const float* A1;        // packed skip_projection [C x C], bias b1
    const float* b1;
    const float* A2;        // packed output_projection [F*M x C], bias b2
    const float* b2;
    const float* A3;        // packed input_projection [C x F*M], bias b3 (used when next_src >= 0)
    const float* b3;
    const float* skip;      // running skip sum [B][C][Ts]
    float* xh;              // the next evaluation's layer-0 input [B][C][Ts]
    long x_bstride;
    int Ts, T, FM;
    float in_scale;         // sqrt(L): the staged skip sum is divided by it (wavenet.py:96)
    int tiles_per_b;
    float inv_tiles_per_b;
    int nout, next_src;     // solver outputs; which of them is the next evaluation's input (-1: none - no input projection)
    float* dst[kMaxOut];    // output o = cm[o] * eps + sum of its terms (in the program's order)
    float cm[kMaxOut];
    int nq;
    EdgeTerm q[kEdgeMaxTerms];
    long o_bstride;         // state buffers: floats between batch items / rows
    int o_rstride;
    const int* cgmap;       // ragged batches: the (item, frame tile) list of this tile width
    int ncg;
};
hipError_t launch_wn_edge(const WnEdgeP& p, int C, int ncb, int nwg, hipStream_t st);
bool wn_edge_supported(int C, int FM);

// lynx_layer.hip: LYNXNet's two pointwise GEMMs with the whole K extent of a 32-frame tile resident in LDS (batched grids)
struct LxLayerP {
    const float* A1;        // packed pw1 weights (PackedGemm, pairC = inner; LayerNorm affine folded in)
    const float* bias1;     // [2 inner]
    const float* A2;        // packed pw2 weights
    const float* bias2;     // [C]
    const float* xin;       // pw1 input: the layer's pre-LayerNorm activations [B][C][Ts]
    const float* stats;     // [B][2][Ts]: mean, rstd per frame (ln_merge_kernel) - read by no kernel since both pw1 forms merge
    const float* lnpart_in; // the producer's LayerNorm partials of xin (same layout as lnpart) - lx_pw1_kernel / lx_pw1p_kernel
                            // merge them themselves
    float* u;               // pw1 output [B][inner][Ts]
    const float* v;         // pw2 input (depthwise conv output) [B][inner][Ts]
    float* x;               // residual stream [B][C][Ts]: read and replaced by pw2
    float* xin_out;         // the NEXT layer's pre-LayerNorm input (nullptr after the last layer)
    const float* cpn;       // next layer's hoisted conditioner projection rows [C][Ts] (nullptr after the last layer)
    long cpn_bstride;
    const float* film;      // next layer's step projection: d[c] = film[c * film_cstride + film_col0 + b * film_colb]
    int film_cstride, film_col0, film_colb;
    float* lnpart;          // [B][C / 64][2][lnpart_ts]: per 64-row tile mean and sum of squared deviations of xin_out
    int lnpart_ts, ln_tiles;
    int ln_rows;            // the rows of xin a LayerNorm counts: C, or fewer (above C - 32) when the last channels are zero padding
                            // (api.hip, pad_weights) - partials in and out carry n_i = min(64, ln_rows - 64 i) rows per tile
    long x_bstride, u_bstride;
    int inner, Ts, T, tiles_per_b, nft, strong;
    float inv_tiles_per_b, inv_nft;     // inv_nft = 1 / (ragged ? ncg : nft)
    const int* cgmap;       // ragged batches: the (item, 32-frame tile) column groups that hold valid frames
    int ncg;
    int rt_groups;          // lx_pw1p_kernel: workgroups per frame tile, each looping over (2 inner / 512) / rt_groups row tiles (0 / 1: one)
};
// which: 0 = pw1, 1 = pw2;  pw1p: DSD_LYNX_PW1P;  cus: compute units of the device (pw1's row-tile groups)
hipError_t launch_lx_layer(const LxLayerP& p, int which, int C, int pw1p, int cus, hipStream_t st);
bool lx_layer_supported(int C, int inner);
// DSD_LYNX_PW1P = force: -1 (by rounds), 0 (lx_pw1_kernel) or a row-tile group count g that divides 2 inner / 512 and is below it
bool lx_pw1p_force_ok(int inner, int force);
hipError_t launch_lx_pw2q(const LxLayerP& p, int C, hipStream_t st);      // pw2 with 128 rows per workgroup: one-utterance grids
bool lx_pw2q_supported(int C, int inner);

// lynx_x3.hip: the two pointwise GEMMs in split-bf16 arithmetic (opt-in precision mode); p.A1 / p.A2 = the layer's bf16x3 weight
// streams [row tile][wave][k32 step][row block][hi | lo][lane][8 bf16]
hipError_t launch_lx_x3(const LxLayerP& p, int which, int C, int ncb, hipStream_t st);     // ncb: 2 = 32-frame tiles, 4 = 64-frame tiles
bool lx_x3_supported(int C, int inner);

// aux_kernels.hip
hipError_t launch_pack(const float* src, long sb, long sr, long st, float* dst, int B, int R, int T, int Ts,
                       hipStream_t stream);
hipError_t launch_unpack(const float* src, int Ts, float* dst, int B, int F, int M, int T, int transpose,
                         const float* scale, const float* shift, hipStream_t stream);
hipError_t launch_transpose(const float* src, int rows, int cols, int src_stride, float* dst, int dst_stride, hipStream_t st);
hipError_t launch_sinemb(const float* t_dev, int ncols, int colstride, const float* freqs, int C, float* dst,
                         hipStream_t stream);
hipError_t launch_lynx_pre(float* x, float* xin, const float* cp, long cp_bstride, const float* film,
                           int film_cstride, int film_col0, int film_colb, long bstride, int rstride, int C, int B,
                           int T, int strong, float* stats, int ts, float eps, hipStream_t stream);
// tconv.hip: time-major MFMA convolution for 16 / 32 channels
struct TConvP {
    const float* W;         // B fragments [tap][CI/4][CO/16][64]: lane l = W[o = nb*16 + (l&15)][c = c4*4 + (l>>4)][tap]
    const float* bias;      // [co_real]
    const float* x;         // input, internal layout
    long x_bstride;
    int x_rstride;
    float* out;
    const float* res;       // residual added after the activation, same layout as out (may alias it), or nullptr
    long o_bstride;
    int o_rstride;
    int T, Ts_out;
    int taps, dil;
    int HP, SP;             // staged halo (multiple of 4) and LDS row stride (16 mod 32)
    float slope_in;         // leaky ReLU on the input (1 = none)
    int act;                // ACT_NONE / ACT_LRELU / ACT_TANH on the output (before the residual)
    int co_real;            // output channels actually stored
    int lds_bytes;
    // ragged batch (dsd_vocode_ragged; cgmap == nullptr: dense): the grid is the ncg (item, 256-frame tile) entries of cgmap,
    // each b * tiles + tile, and item b's input frames t >= lens[b] are zero padding
    const int* lens;
    const int* cgmap;
    int ncg, tiles;
};
int tconv_lds_bytes(int ci, int co, int taps, int SP);
hipError_t launch_tconv(const TConvP& p, int ci, int co, int batch, hipStream_t st);
// voc_x3.hip: a residual-block convolution Conv1d(C -> C, k taps, dilated) of the vocoder in split-bf16 arithmetic (opt-in
// precision mode):  out = lrelu(bias + W * lrelu(x, slope_in), slope_out) (+ res), a slope of 1 = no activation
struct VocX3P {
    const void* W;          // bf16x3 weight stream [wave 4][k32 step = tap * C/32 + chunk][row block][hi | lo][lane][8 bf16]
    const float* bias;      // [C]
    const float* x;         // input, internal layout [B][C][Ts]
    const float* res;       // residual added last, same layout (may be x), or nullptr
    float* out;             // same layout; never x or res (neighbouring tiles read their halo)
    long bstride;           // floats between batch items: C * Ts
    int Ts, T, C, taps, dil;
    int HL;                 // staged halo frames on each side: (taps / 2) * dil rounded up to 4
    int nsteps;             // taps * C / 32
    int nfq;                // staged frame quads: (tile width + 2 HL) / 4
    float inv_nfq;
    float slope_in, slope_out;
    int tiles_per_b;
    float inv_tiles_per_b;
    const int* lens;        // ragged batch: per-item valid frames (nullptr: T)
    const int* cgmap;       // ragged batch: the (item, tile) entries b * tiles_per_b + tile with valid frames, of this tile width
    int ncg;
};
int voc_x3_mbw(int C);                              // 16-row blocks per wave: the stream holds 4 * voc_x3_mbw(C) * 16 rows, zero above C
int voc_x3_max_ncb(int C, int taps, int dil);       // widest tile in 16-frame blocks (4 or 2) whose LDS images fit; 0: not supported
hipError_t launch_voc_x3(const VocX3P& p, int ncb, int ntiles, hipStream_t st);
// vocoder_kernels.hip (NSF-HiFiGAN source, noise convs, residual-block average)
hipError_t launch_voc_source(const float* f0, const float* rand_ini, const float* noise, const float* lin_w,
                             const float* lin_b, int B, int T, int upp, int dim, float sr, float sine_amp, float noise_std,
                             float* acc_tmp, int Tsu, float* har, hipStream_t st, const int* lens = nullptr);
hipError_t launch_voc_add_noise(float* x, const float* noise, int B, int C, int T, int Ts, float sigma, hipStream_t st,
                                const int* lens = nullptr);
hipError_t launch_voc_fast_source(const float* f0, int B, int T, int upp, float source_sr, float* acc_tmp, int Tsu, float* har,
                                  hipStream_t st, const int* lens = nullptr);
constexpr int VOC_NOISE_NQ = 16;                    // frames per thread of the noise conv
int voc_noise_groups(int C, int sf, int ksz);       // frame groups per workgroup whose source window fits in LDS; 0: none does
// lens_q / lens_up (ragged: per-item output frames / source samples) both or neither
hipError_t launch_voc_noise_conv(float* x, const float* har, const float* w, const float* bias, int B, int C, int Tq,
                                 int Tsq, int sf, int ksz, long Tup, int Tsu, hipStream_t st, const int* lens_q = nullptr,
                                 const int* lens_up = nullptr);
hipError_t launch_voc_accum(float* acc, const float* r, long n, int first, float div, hipStream_t st);
// encoder_kernels.hip (FastSpeech2 acoustic encoder glue)
struct EncExpandArgs {
    const float* lin_w[7];
    const float* lin_b[7];
    const float* feat[7];
    const float* spk_table;
    const long long* spk_id;
    const float* spk_mix;
    long spk_mix_bstride, spk_mix_tstride;
    int num_spk;
};
struct AssembleArgs {             // dsd_cond_assemble, device view
    int B, T, H, n_gather, n_terms;
    const float* g_table[4];
    long g_bstride[4], g_rows[4], g_off[4];
    const long long* g_idx[4];
    float g_scale[4];
    const float* g_rowscale[4];
    const float* t_s[16];
    const float* t_v[16];
};
hipError_t launch_enc_sinpos(float* x, const float* nonpad, const float* freqs, int C, int B, int L, int Ls, hipStream_t st);
hipError_t launch_enc_relpos(float* x, const float* div, int C, int B, int L, int Ls, hipStream_t st);
hipError_t launch_enc_nonpad(const unsigned char* pad, int B, int L, int Ls, float* nonpad, hipStream_t st);
hipError_t launch_enc_dur_head(const float* x, const float* w, const float* bias, const float* nonpad, int C, int B, int L,
                               int Ls, float offset, float* dur, hipStream_t st);
hipError_t launch_assemble(const AssembleArgs& a, float* out, hipStream_t st);
hipError_t launch_enc_dur(const long long* mel2ph, int B, int T, int L, int* dur, hipStream_t st);
hipError_t launch_enc_embed(const long long* tokens, const long long* langs, const int* dur, const float* txt_embed,
                            int vocab, const float* lang_embed, int n_lang_rows, const float* dur_w, const float* dur_b,
                            float embed_scale, int H, int B, int L, int Ls, float* x, float* nonpad, hipStream_t st);
hipError_t launch_enc_layernorm(const float* x, float* y, const float* g, const float* beta, const float* mask, int C,
                                int B, int L, int Ls, float eps, hipStream_t st);
hipError_t launch_enc_mask(float* x, const float* mask, int C, int B, int L, int Ls, hipStream_t st);
// SwiGLU between ffn_1 and ffn_2: x[b][c][l] *= silu(x[b][half + c][l]) for c < half (common_layers.py:107-117)
hipError_t launch_enc_swiglu(float* x, int half, long bstride, int B, int L, int Ls, hipStream_t st);
hipError_t launch_enc_rope(float* qkv, const float* freqs, int H, int head_dim, int B, int L, int Ls, hipStream_t st);
hipError_t launch_enc_attention(const float* qkv, const float* nonpad, float* out, int H, int heads, int B, int L, int Ls,
                                hipStream_t st);
hipError_t launch_enc_expand(const float* enc, const long long* mel2ph, const EncExpandArgs& a, int H, int B, int L, int Ls,
                             int T, float* cond, hipStream_t st);
// (C = the rows the LayerNorm counts: tile i holds min(64, C - 64 i) of them, which may leave mtiles * 64 above C)
hipError_t launch_ln_merge(const float* lnpart, int mtiles, int C, int B, int T, int ts, float eps, float* stats,
                           hipStream_t stream);
hipError_t launch_dwconv(const float* src, float* dst, long bstride, int rstride, int C, int B, int T, const int* lens,
                         const float* w, const float* bias, int ksz, int act, const float* prelu, hipStream_t stream);

// frames_kernels.hip: durations -> frames (dsd_length_regulate) and the smoothed frame-level MIDI curve with its retake
// blend (dsd_frame_curve).  A FrameCurveP launch covers up to kCurveItems batch items starting at item b0; the smoothing
// taps and the items' lengths travel in the kernel arguments, so neither entry owns device memory.
constexpr int kRegulateMaxTokens = 2048;    // the encoders' own token limit
constexpr int kCurveMaxTaps = 255;
constexpr int kCurveItems = 64;
struct FrameCurveP {
    const float* note_midi;         // [B][N]
    const long long* mel2note;      // [B][T]
    const float* pitch;             // [B][T]
    const unsigned char* retake;    // [B][T]
    float *base, *blend, *delta;    // [B][T] each
    int N, T, K, b0;
    int len[kCurveItems];
    float w[kCurveMaxTaps];
};
hipError_t launch_length_regulate(const long long* dur, int B, int L, int T, long long* mel2x, hipStream_t st);
hipError_t launch_frame_curve(const FrameCurveP& p, int items, hipStream_t st);

// stage_kernels.hip: the index and per-frame scalar work of the variance twin's stages (dsd_variance_*), between the
// length regulator and the assemble kernel.  Plain launches on tiny grids; every output is a workspace block of the object.
struct StageEncodeP {               // forward_linguistic_encoder_word / _phoneme
    const long long* tokens;        // [B][L]
    const long long* ph2word;       // [B][L], or nullptr: the phoneme form
    const long long* word_dur;      // [B][W]
    const long long* ph_dur;        // [B][L] (phoneme form)
    const long long* languages;     // [B][L] or nullptr
    const float* mask;              // [vocab] 0 / 1
    int L, W, vocab;
    long long* onset;               // [B][L]
    long long* lang;                // [B][L]
    float* dur_f;                   // [B][L]
    unsigned char* x_masks;         // [B][L]
};
struct StageNoteP {                 // MelodyEncoder.forward's terms
    const float* note_midi;         // [B][N]
    const unsigned char* note_rest;
    const long long* note_dur;
    const long long* note_glide;    // or nullptr (zeros)
    int N;
    float scale;                    // sqrt(melody hidden size)
    float *midi_s, *keep_s, *dur_f; // [B][N] each
    long long* glide;               // [B][N]
    unsigned char* pad;             // [B][N]: note_midi < 0
};
struct StageFrameP {                // per-frame scalars of the two condition stages, and the speaker gather's index
    int T, V;                       // V > 0: the variance form
    const float* expr;              // [B][T] or nullptr        (pitch form)
    const unsigned char* retake;    // [B][T] or [B][T][V]
    const float* curves[4];         // [B][T] each              (variance form)
    float *e, *one_minus_e;         // [B][T]                   (pitch form)
    float *keep[4], *kept[4];       // [B][T] each: !retake, curve * !retake
    long long* spk_idx;             // [B][T]: t (spk_iota) or 0; nullptr: not wanted
    int spk_iota;
};
struct StagePostP {
    const float* sample;            // [B][F][T][M]
    const float* base;              // [B][T] or nullptr
    float* out[4];                  // [B][T] per curve
    int F, T, M;
    float lo[4], hi[4];
    int clamp[4];
};
hipError_t launch_stage_encode(const StageEncodeP& p, int B, hipStream_t st);
hipError_t launch_stage_iota(long long* iota, long long* spk_idx, int spk_iota, int B, int L, hipStream_t st);
hipError_t launch_stage_notes(const StageNoteP& p, int B, hipStream_t st);
hipError_t launch_stage_frames(const StageFrameP& p, int B, hipStream_t st);
hipError_t launch_stage_post(const StagePostP& p, int B, hipStream_t st);

// acoustic_kernels.hip: the per-token and per-frame work of the acoustic twin's condition stage (dsd_acoustic_condition),
// the samplers' start state and the mel base.  Plain launches; every output but x and mel is a workspace block of the object.
struct AcTokensP {
    const long long* tokens;        // [B][L]
    const long long* durations;     // [B][L]
    const long long* languages;     // [B][L], or nullptr: lang = 0
    const float* mask;              // [vocab] 0 / 1
    int L, vocab;
    long long* dur_m;               // [B][L]: durations * (tokens > 0)
    long long* lang;                // [B][L], or nullptr: the model has no lang_embed
};
struct AcFramesP {
    const long long* mel2ph;        // [B][T]
    const float* f0;                // [B][T]
    const float* gender;            // [B][T]; read when key_shift is wanted and there is no frozen value
    const float* velocity;          // [B][T] or nullptr (speed = 1)
    const float* frozen_key_shift;  // device, 1 value, or nullptr
    int T;
    float shift_max, shift_min_abs, speed_min, speed_max;
    float inv_700, coarse_a, coarse_b;      // f0_to_coarse's constants, rounded to fp32 as torch rounds Python scalars
    float* f0_m;                    // [B][T]: f0 * (mel2ph > 0)
    float* f0_enc;                  // [B][T] or nullptr: what the encoder takes - f0_m, or zeros with `coarse`
    float* key_shift;               // [B][T] or nullptr
    float* speed;                   // [B][T] or nullptr
    long long* iota;                // [B][T] or nullptr: t
    long long* coarse;              // [B][T] or nullptr: f0_to_coarse(f0_m)
    long long* coarse_out;          // the caller's copy of it, or nullptr
};
hipError_t launch_ac_tokens(const AcTokensP& p, int B, hipStream_t st);
hipError_t launch_ac_frames(const AcFramesP& p, int B, hipStream_t st);
// source [B][T][M] -> x [B][1][M][T] = (source - mid[m]) / k[m]; with `noise` ([B][1][M][T]): src_scale * that + noise_scale * noise
hipError_t launch_ac_source(const float* source, const float* noise, const float* k, const float* mid, float src_scale, float noise_scale,
                            int B, int M, int T, float* x, hipStream_t st);
hipError_t launch_ac_mel_base(float* mel, long n, float scale, hipStream_t st);

// spk_mix_kernels.hip: out[b][r][:] = sum_n w[b][r][n] * table[ids[b][n]][:] (dsd_acoustic_spk_mix, dsd_variance_spk_mix)
struct SpkMixP {
    const float* table;             // [num_spk][H]
    const int* ids;                 // device [B][N], each a row of `table` (the host entry has checked them)
    const float* values;            // [B][rows][N]
    float* out;                     // [B][rows][H]
    int rows, N, H, normalize;
    int lanes;                      // the launcher's: lanes per row, a power of two <= 256
};
hipError_t launch_spk_mix(SpkMixP p, int B, hipStream_t st);

// noise_kernels.hip: seeded draws (dsd_noise_fill).  A NoiseP launch covers up to kNoiseItems batch items starting at item
// b0; their seeds travel in the kernel arguments, so the entry owns no device memory and never synchronises.
constexpr int kNoiseItems = 64;
struct NoiseP {
    float* out;                     // [n][B][rows][cols]
    const float* src;               // the same layout, or nullptr
    float scale, src_scale;         // out = src_scale * src + scale * eps
    unsigned domain, first_stream;
    int n, B, rows, cols, b0, kind; // kind: 0 normal, 1 uniform
    unsigned long long seed[kNoiseItems];
};
hipError_t launch_noise_fill(const NoiseP& p, int items, hipStream_t st);
// vocoder_kernels.hip, the seeded forms (dsd_vocode_seeded): the source and pre-noise kernels draw what dsd_noise_fill would have
// written under these domains (include/dsdenoise.h: DSD_DOMAIN_VOC_*), stream 0, scale 1.  Seeds as in NoiseP: by value, up to
// kNoiseItems items from b0 per launch.  `seeds` is a HOST array of B values.
constexpr unsigned kVocSourceDomain = 3, kVocPreDomain = 4, kVocPhaseDomain = 5;
struct VocSeedP {
    int b0;
    unsigned long long seed[kNoiseItems];
};
hipError_t launch_voc_source_seeded(const float* f0, const float* rand_ini, const unsigned long long* seeds, const float* lin_w,
                                    const float* lin_b, int B, int T, int upp, int dim, float sr, float sine_amp,
                                    float noise_std, float* acc_tmp, int Tsu, float* har, hipStream_t st, const int* lens);
hipError_t launch_voc_add_noise_seeded(float* x, const unsigned long long* seeds, int B, int C, int T, int Ts, float sigma,
                                       hipStream_t st, const int* lens);

// score_kernels.hip: validation scoring (dsd_diffuse, dsd_masked_loss, dsd_curve_stats, dsd_dur_score).  The reductions
// sum doubles in an order fixed by the element count alone (include/dsdenoise.h, "the rounding rule"): workgroup g of
// score_blocks(n) takes the spans g, g + G, ... of kScoreSpan elements; its sums go to slot-major partials in the caller's
// workspace, [kScoreSlots][kScoreMaxBlocks] 8-byte values, and a one-workgroup launch adds those.
constexpr int kScoreThreads = 256;
constexpr int kScoreSpan = 2048;
constexpr int kScoreMaxBlocks = 1024;
constexpr int kScoreSlots = 8;
inline int score_blocks(long long n) {
    const long long spans = (n + kScoreSpan - 1) / kScoreSpan;
    return (int)(spans < kScoreMaxBlocks ? spans : kScoreMaxBlocks);
}
struct DiffuseP {                   // a launch covers up to kNoiseItems items from b0, as NoiseP
    float* x_t;
    float* target;                  // or nullptr
    const float* x0;
    const float* eps;               // or nullptr: drawn from seed[]
    const float* a;
    const float* c;
    unsigned domain;
    int rows, cols, b0, kind;       // kind: 0 ddpm, 1 reflow
    unsigned long long seed[kNoiseItems];
};
hipError_t launch_diffuse(const DiffuseP& p, int items, hipStream_t st);
struct LossP {
    const float* pred;
    const float* target;
    const float* non_padding;       // or nullptr
    const float* t;                 // or nullptr
    int B, rows, cols, kind;        // kind: 0 l1, 1 l2
};
hipError_t launch_masked_loss(const LossP& p, void* ws, double* out, hipStream_t st);
hipError_t launch_curve_stats(const float* pred, const float* target, const unsigned char* mask, long long n, float tol, void* ws,
                              void* out, hipStream_t st);
struct DurP {
    const float* dur_pred;
    const float* dur_gt;
    const long long* ph2word;
    const unsigned char* mask;      // or nullptr
    float* wdur_pred;               // [B][n_words - 1]
    float* wdur_gt;
    int B, L, n_words, kind;        // kind: 0 mse, 1 huber
    float offset, tol_rhythm, tol_pdur;
};
hipError_t launch_dur_score(const DurP& p, void* ws, void* out, hipStream_t st);

// track_kernels.hip: a project's track (dsd_track_place / _peak / _export).  One workgroup covers kTrackSpan consecutive
// samples of the track: 256 threads, each one 16-byte aligned pair of doubles (diffsinger_amd/track.py: SPAN).  The
// launchers take the stream as void* and answer nullptr or hipGetErrorString's text, so that track_api.hip - the plan and
// every argument check - stays free of HIP headers and compiles with a plain host compiler (tools/harness/track_harness.cpp).
constexpr int kTrackSpan = 512;
const char* launch_track_place(double* track, long long start, long long prev_end, const float* src, long long n, void* stream);
const char* launch_track_peak(const double* track, long long total, double* peak_out, void* stream);
const char* launch_track_export(const double* track, long long total, int kind, const double* peak, void* out, void* stream);

// The DFT tile of mel_dft_kernel and hs_dft_kernel (dsd_device.h, dft_tile_walk), as far as the host sizes bases and work
// lists by it
constexpr int kDftFrames = 64;      // frames per tile (one work-list entry)
constexpr int kDftRows = 64;        // basis rows per tile: a basis holds a multiple of them
constexpr int kDftTaps = 32;        // taps staged per chunk: a basis row holds a multiple of them

// mel_kernels.hip: waveform -> log-mel (dsd_mel_analyze).  work: 5 ints per (item, 64-frame tile) entry = item b, first
// frame t0, item length L in samples, item frame count T_b, index of the entry's first frame in the magnitude buffer
struct MelDftP {
    const float* wav;
    long wav_bstride;
    const int* work;
    const float* basis;     // [row tiles * kDftRows][Kpad] (mel_basis_kernel)
    int Kpad, W, H, off, padL;
    int nb;                 // bins computed: k_lo .. k_lo + nb - 1
    int rescale;            // keyshift != 0: |X| * win_size / W'
    float win_size, win_new;
    float* mags;            // [nb][G]
    long G;                 // frames of the whole call
};
struct MelProjP {
    const int* work;
    const float* mags;
    long G;
    int nb, M;
    const int* range;       // [M][2]: bins [lo, hi) relative to k_lo
    const int* woff;        // [M]: offset of filter m's packed weights in fw
    const float* fw;
    float clip;
    float* out;
    long o_sb, o_sm, o_st;
};
hipError_t launch_mel_basis(float* basis, int Rpad, int Kpad, int k_lo, int nb, int N, int W, int off, hipStream_t st);
hipError_t launch_mel_dft(const MelDftP& p, int n_entries, int row_tiles, hipStream_t st);
hipError_t launch_mel_project(const MelProjP& p, int n_entries, hipStream_t st);

// rmvpe_kernels.hip: RMVPE pitch extraction (dsd_rmvpe_*).  work lists: 3 ints per (item, tile) entry = item b, first
// quad / position / frame of the tile, the item's extent at that level (frames; Tin for the transposed conv).
// Activations: [b][t < Tal][F][C] floats, Tal = the call's largest padded frame count at that level.
struct RmResampleP {
    const float* x;
    long x_sb;
    const int *len_in, *len_out;    // [B] samples in / out per item
    const float* kern;              // [nw][K]
    int K, orig, nw, width;
    float* y;
    long y_sb;
};
struct RmPrepP {
    const float* mel;               // element (b, m, t) at mel[b sb + m sm + t st]
    long sb, sm, st;
    const int *T, *Tp;              // [B] frames, padded frames
    float scale, shift;             // unet.encoder.bn
    float* x;                       // [b][Tal][128]
    int Tal;
};
struct RmConvP {
    const float *x0, *x1;           // conv input: x0 (c0 channels) then x1 (c1 channels, 0 = none): torch.cat(dim=1)
    int c0, c1;
    const float *r0, *r1;           // residual input (the ConvBlockRes input), rc0 + rc1 channels
    int rc0, rc1;
    int res_mode;                   // 0 none, 1 identity (rc0 == cout), 2 shortcut conv ws / bs
    const float* w;                 // [tap][c0 + c1][cout_pad], BN scale folded in
    const float* shift;             // [cout_pad]: BN shift or the conv bias
    const float *ws, *bs;           // [rc0 + rc1][cout_pad], [cout_pad]
    int cout, cout_pad, relu;
    int F, Tal;                     // bins and allocated frames of the INPUT level
    float* y;                       // [b][Tal][F][cout] (the transposed conv: [b][2 Tal][2 F][cout])
    float* pool;                    // optional AvgPool2d(2) of y: [b][Tal / 2][F / 2][cout]
    const int* work;
};
struct RmLinearP {
    const float* x;                 // [b][Tal][K]
    const float* w;                 // [K][N]
    const float* bias;              // [N]
    int K, N, act, Tal;
    float* y;                       // [b][Tal][N]
    const int* work;                // (b, t0, Tp_b)
};
struct RmGruP {
    const float* gi;                // [b][Tal][1536]
    const float* whh;               // [2][256][768]: W_hh transposed per direction
    const float* bhh;               // [2][768]
    const int* Tp;
    int Tal;
    float* y;                       // [b][Tal][512]
};
struct RmDecodeP {
    const float* hidden;            // frame (b, t) at hidden + b h_sb + t h_st, 360 contiguous classes
    long h_sb, h_st;
    const int* T;
    int B, Tmax;
    float thred;
    float* f0;                      // optional: f0[b f_sb + t]
    long f_sb;
    float* out_hidden;              // optional copy, [b o_sb + t o_st + class]
    long o_sb, o_st;
    const int* center;              // optional: the window's centre of frame (b, t) at center[b c_sb + t]; null = the argmax
    long c_sb;
};
// Viterbi decode: the band of the transition matrix is 59 wide (|k - j| <= 29)
constexpr int RM_VT_BAND = 29, RM_VT_W = 2 * RM_VT_BAND + 1;
struct RmViterbiP {
    const float* hidden;            // as RmDecodeP
    long h_sb, h_st;
    const int* T;
    int B, Tmax;
    const double* tab;              // [59][360]: tab[d + 29][j] = log_trans[j + d][j] (0 where j + d is no state)
    double eps, log_eps, log_p_init;
    double* lp;                     // workspace [b][Tmax][360]: log_prob
    unsigned short* ptr;            // workspace [b][Tmax][360]: back-pointers (row 0 unused)
    int* center;                    // [b][Tmax]: the path
    int* path_out;                  // optional copy: path_out[b p_sb + t]
    long p_sb;
};
hipError_t launch_rm_resample(const RmResampleP& p, int B, long max_blocks, int nw, hipStream_t st);
hipError_t launch_rm_prep(const RmPrepP& p, int B, int Tal, hipStream_t st);
hipError_t launch_rm_conv3(const RmConvP& p, int n_entries, hipStream_t st);
hipError_t launch_rm_tconv(const RmConvP& p, int n_entries, hipStream_t st);
hipError_t launch_rm_linear(const RmLinearP& p, int n_entries, hipStream_t st);
hipError_t launch_rm_gru(const RmGruP& p, int B, hipStream_t st);
hipError_t launch_rm_decode(const RmDecodeP& p, hipStream_t st);
hipError_t launch_rm_viterbi(const RmViterbiP& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// hnsep_kernels.hip: VR harmonic-noise separation and the variance curves
// ---------------------------------------------------------------------------------------------
struct HsView {                     // element (b, f, t, c) at p + b bs + f fs + t ts + c cs
    float* p;
    long bs, fs, ts, cs;
};
struct HsSrc {                      // a conv source: C channels (Cp = C rounded up to 4) at p + b bs + f fs + t ts + c cs
    const float* p;
    long bs, fs, ts, cs;
    int C, Cp;
    int mode;                       // 0 plain, 1 bilinear x2 upsample (align_corners), 2 one bin broadcast over bins
};
struct HsConvP {
    HsSrc src[4];
    int nsrc;
    const float* w;                 // [(source, tap kf * ks + kt, channel < Cp)][cout_pad], BN scale folded
    const float* shift;             // [cout_pad]
    HsView y;
    int cout, cout_pad;
    int F, Fin;                     // output / input bins
    int ks, stride, dil_f, dil_t;
    int act;                        // 0 none, 1 ReLU, 2 LeakyReLU(0.01)
    const int* work;                // (b, q0, T_l out, T_l in)
};
struct HsBinMeanP {
    HsView x, y;
    int F, C;
    const int* T;
};
struct HsLstmNet {
    const float* gi;                // [b][t][2][4H]
    long gi_bs;
    const float* whh;               // [2][4H][H]
    float* y;                       // [b][t][2][H]
    long y_bs;
    int H;
};
struct HsLstmP {
    HsLstmNet net[2];
    const int* T;
};
struct HsMaskP {
    HsView x, y;                    // the out conv (channels re 0..C-1, im C..2C-1) -> the mask (re at c cs, im at y_im + c cs)
    long y_im;
    int F, Fx, C;                   // mask bins, conv bins (the last one replicated)
    const int* T;
};
// hs_dft_kernel<0 / 1>.  The spectrum of both directions: element (b, bin, t) at + b s_sb + bin s_sf + t s_st, re at channel
// ch, im at channel s_cim + ch.  work: 6 ints per (item, 64-frame tile, channel) entry = b, t0, L, T_b, ch, padL (forward).
struct HsStftP {
    const float* basis;             // [row tiles * 64][N] (hs_basis_kernel, forward)
    int N, nb;
    const float* wav;               // channel ch of item b at wav + b wav_sb + ch wav_sc
    long wav_sb, wav_sc;
    int H, reflect;                 // hop; outside the item: 0 zeros (pad_mode 'constant'), 1 torch's 'reflect'
    float* spec;
    long s_sb, s_sf, s_st;
    int s_cim, nrep;                // nrep > 1: one clip written to channels ch .. ch + nrep - 1 (wav_sc = 0)
    const int* work;
};
struct HsIstftP {
    const float* basis;             // [row tiles * 64][Kpad] (hs_basis_kernel, inverse)
    int Kpad, N, nb;
    const float* spec;
    long s_sb, s_sf, s_st;
    int s_cim;
    const float* mask;              // the network's mask (NULL: the f0 bin mask): (b, bin, t) at + b m_sb + bin m_sf + t m_st,
    long m_sb, m_sf, m_st;          // re / im at channel ch / m_cim + ch, mask_F bins (the last one replicated)
    int m_cim, mask_F;
    const float* f0;                // [b f0_sb + t], f0_len[b] frames
    long f0_sb;
    const int* f0_len;
    float sr, half_width;
    float* frames;                  // [(b nch + ch) f_sb + t N + j]
    long f_sb;
    int nch;
    const int* work;
};
struct HsOlaP {
    const float* frames;            // [(b nch + c) f_sb + t N + j]
    long f_sb;
    const float* win;
    int N, H, nch;
    const int* T;                   // frames per item
    const long* len;                // output samples per item
    const long* off0;               // padded position of output sample 0
    float* out;
    long o_sb, o_sc;                // o_sc 0: the mean of the channels at out + b o_sb; else channel c at + c o_sc
};
struct HsRmsP {
    const float *wav, *harm, *base; // any may be NULL
    long sb;
    const long* len;
    const int* nfr;                 // librosa frames per item: 1 + L // hop
    int hop, win, B, Tmax;
    float* rms;                     // [4][B][Tmax]
};
struct HsCurvesP {
    const float* rms;
    const int *nfr, *length;
    int B, Tmax, domain, db;        // db 0: energy / breathiness / voicing stay RMS
    float* out[4];                  // energy, breathiness, voicing, tension (any may be NULL): [b o_sb + t]
    long o_sb;
};
hipError_t launch_hs_basis(float* basis, const float* win, int Rpad, int Kpad, int nb, int N, int inv, hipStream_t st);
hipError_t launch_hs_stft(const HsStftP& p, int n_entries, int row_tiles, hipStream_t st);
hipError_t launch_hs_istft(const HsIstftP& p, int n_entries, int row_tiles, hipStream_t st);
hipError_t launch_hs_ola(const HsOlaP& p, int B, long max_len, hipStream_t st);
hipError_t launch_hs_conv(const HsConvP& p, int n_entries, hipStream_t st);
hipError_t launch_hs_binmean(const HsBinMeanP& p, int B, int Tmax, hipStream_t st);
hipError_t launch_hs_lstm(const HsLstmP& p, int B, int nnet, hipStream_t st);
hipError_t launch_hs_mask(const HsMaskP& p, int B, int Tmax, hipStream_t st);
hipError_t launch_hs_rms(const HsRmsP& p, hipStream_t st);
hipError_t launch_hs_curves(const HsCurvesP& p, hipStream_t st);

}  // namespace dsd
