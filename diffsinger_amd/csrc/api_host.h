// Private host-side header of libdsdenoise: what api.hip and the analysis families' host sources (mel_api.hip,
// rmvpe_api.hip, hnsep_api.hip) share - the handle, error reporting, the entry check of every call that takes a handle
// (enter) and the prologue of every create, device-memory ownership, weight loading.  No kernels.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <vector>

#include "../../include/dsdenoise.h"
#include "dsd_internal.h"
#include "ragged_tiles.h"

using namespace dsd;

struct dsd_handle;

namespace dsd {

// records the message on the handle (h == nullptr: for dsd_last_error(NULL), as the create functions do) and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);

#define HIP_OK(h, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(h, DSD_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)


// Device memory that its holder owns and only ever grows: reserve(n) keeps the allocation while n elements fit, otherwise
// frees it and allocates anew (the contents are not carried over, and the address changes: whoever gave the old one to a
// captured graph destroys that graph).  Move-only, so a std::vector of holders keeps the device addresses when it grows.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;         // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int reserve(dsd_handle* h, size_t n, const char* who) {
        if (n <= cap) return DSD_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return fail(h, DSD_ENOMEM, "%s: hipMalloc of %zu bytes failed", who, n * sizeof(T));
        cap = n;
        return DSD_OK;
    }
};

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// one packed GEMM operand set on the device
struct PackedGemm {
    size_t a_off = 0;     // float offset into the weight blob
    size_t bias_off = 0;  // float offset, or SIZE_MAX
    int M = 0;            // real rows
    int K = 0;            // padded input channels
    int Kreal = 0;
    int taps = 1;
    int pairC = 0;        // > 0: paired packing with this many pairs
};

// weights of a few-channel convolution in tconv.hip's B-fragment order
struct PackedTConv {
    size_t w_off = SIZE_MAX, b_off = 0;
    int ci = 0, co = 0, co_real = 0, taps = 0;
    bool valid() const { return w_off != SIZE_MAX; }
};

struct GraphEntry {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// A ragged batch's host block, its copy on the device and the key both were built for: build_ragged's output for (B, T, lengths)
// at every rate of `mult`, and the grids over it.  build() is host work only; upload_ragged (api.hip) puts the block on the
// device before the first launch that reads it - on the caller's stream, outside any capture - and destroys the cached graphs
// when the block had to move.  The same key always gives the same offsets, so while the block stays where it is a graph
// captured for a key finds its lists at the addresses and with the contents it was captured with.
struct RaggedOwner {
    std::vector<int> key;               // {B, T, lengths...} of `host` (empty: nothing built)
    std::vector<int> host;
    DevBuf<int> dev;
    size_t dense = 0;                   // what `dev` reserves: the block of this (B, T) with every item T long
    bool on_device = false;             // `dev` holds `host`
    bool active = false;                // the denoiser side: dsd_set_lengths gave lengths (NULL clears it, the block stays)
    std::vector<RaggedGrid> grids;      // per rate; upload_ragged points them at the device copy
    const RaggedGrid* grid(size_t rate = 0) const { return active ? &grids[rate] : nullptr; }
    const int* lengths() const { return key.data() + 2; }
    bool built_for(const int* lengths, int B, int T) const {
        return key.size() == (size_t)B + 2 && key[0] == B && key[1] == T && std::equal(lengths, lengths + B, key.begin() + 2);
    }
    // `lengths` may be this owner's own (a rebuild at another T)
    void build(const int* lengths, int B, int T, unsigned widths, const std::vector<long>& mult, bool nb_by_valid_tiles,
               bool mask_every_gemm) {
        std::vector<int> k = {B, T};
        k.insert(k.end(), lengths, lengths + B);
        key.swap(k);
        dense = build_ragged(this->lengths(), B, T, widths, mult, host, grids);
        for (RaggedGrid& g : grids) { g.nb_by_valid_tiles = nb_by_valid_tiles; g.mask_every_gemm = mask_every_gemm; }
        on_device = false;
        active = true;
    }
};

// dsd_mel_analyze: per handle, the filterbank on the device and the DFT bases of the (N', W') sizes met so far
struct MelBasis {
    int N = 0, W = 0;
    DevBuf<float> dev;
};
struct MelState {
    dsd_mel_config cfg;
    int k_lo = 0, k_hi = -1;            // the bins any filter reads (k_hi < k_lo: none)
    std::vector<int> range_host;        // [M][2] bins [lo, hi) relative to k_lo
    DevBuf<int> range, woff;
    DevBuf<float> fw;                   // packed non-zero runs
    std::vector<MelBasis> bases;        // most recent last
    std::vector<int> work_host;
    DevBuf<int> work;
    DevBuf<float> mags;
};


// The STFT geometry of one (keyshift, speed) (nvSTFT.py:52-66): np.round is round-half-even, as nearbyint
struct MelGeom {
    int N, W, H, off, padL, padR;
    bool rescale;
};

}  // namespace dsd

struct RmvpeState;
struct HnsepState;

struct dsd_handle {
    dsd_config cfg;
    std::string err;
    std::map<std::string, HostTensor> raw;
    // A channel count that is not a multiple of 32 (any WaveNet; LYNXNet and the aux decoder through dsd_create_any_width):
    // cfg.num_channels is the count the kernels run with (rounded up), c_user the caller's (0: the same); `padded` holds the
    // zero-extended tensors build_packed reads (pad_weights)
    std::map<std::string, HostTensor> padded;
    int c_user = 0;
    // wn_edge.hip: the state buffer whose input projection the previous evaluation's edge kernel already wrote into xh
    const float* edge_xh_src = nullptr;
    bool finalized = false;         // the packed weights are on the device, for every kind that has some (enter() reads it)
    PathOpts opts;                  // path switches: the snapshot of the last entry point that launches kernels (read_path_opts)

    // packed weights
    std::vector<float> blob_host;
    DevBuf<float> blob;
    PackedGemm g_inproj, g_emb0, g_emb1, g_dproj, g_cp, g_tail1, g_out;
    std::vector<PackedGemm> g_conv, g_outp;          // WaveNet per layer
    // fp32 mode: every layer's out-proj once more with the skip projection folded into its skip rows (build_packed); the
    // evaluations that do not end in the edge kernel read it and run no skip-projection GEMM.  Empty: not built (bf16x3 mode)
    std::vector<PackedGemm> g_outf;
    // split-bf16 precision mode (wn_layer_x3.hip): 0 = fp32 (default), 1 = bf16x3 where a kernel exists; the layers' weight
    // streams (float offsets into the blob; empty: not built)
    int precision = 0;
    std::vector<size_t> x3_conv, x3_out;
    int cus = 256;                  // compute units of the device (hipDeviceProp_t::multiProcessorCount): one fused round = `cus` tiles
    std::vector<PackedGemm> g_pw1, g_pw2;            // LYNXNet per layer
    std::vector<size_t> dw_w, dw_b, dw_prelu;        // LYNXNet / ConvNeXt depthwise params (float offsets)
    PackedGemm g_ain, g_aout;                        // ConvNeXt aux decoder: dense k-tap in/out convs
    // NSF-HiFiGAN generator
    dsd_vocoder_config vcfg;
    PackedGemm v_pre, v_post;
    std::vector<PackedGemm> v_ups;                   // transposed convs as phase-row GEMMs
    std::vector<std::vector<PackedGemm>> v_res;      // [stage * n_kernels + j][2 * n_dil (ResBlock1) or n_dil]
    std::vector<std::vector<PackedTConv>> v_rest;    // same indexing: the 16- / 32-channel stages (tconv.hip)
    // split-bf16 mode (precision == 1): same indexing as v_res, the convolution's weight stream of voc_x3.hip as a float offset
    // into the blob, SIZE_MAX where the convolution stays on the fp32 kernel; v_x3_ran: the last vocode call launched voc_x3.hip
    std::vector<std::vector<size_t>> v_resx3;
    bool v_x3_ran = false;
    PackedTConv v_postt;
    std::vector<size_t> v_nw, v_nb;                  // noise conv weights / biases
    std::vector<int> v_uptaps;
    size_t v_linw = 0, v_linb = 0;
    int vB = 0, vT = 0;
    DevBuf<float> v_arena;
    std::vector<float*> v_buf;                       // per stage: x, t1, r, acc
    float *v_mel = nullptr, *v_pre_out = nullptr, *v_har = nullptr, *v_phase = nullptr, *v_wav = nullptr;
    float* v_ini = nullptr;             // dsd_vocode_seeded: the initial phases it draws, [B][harmonic_num + 1]
    // ragged vocoder batches (dsd_vocode_ragged): lengths and valid-tile lists at every rate of the generator
    RaggedOwner vrag;
    // mel analysis (dsd_mel_create): the config, the filterbank's packed non-zero runs and the device blocks of dsd_mel_analyze
    MelState* mel = nullptr;
    // RMVPE pitch extraction (dsd_rmvpe_create): config, packed weights, its own mel front end, workspace
    RmvpeState* pe = nullptr;
    // VR harmonic-noise separation (dsd_hnsep_create): config, packed weights, DFT bases, workspace
    HnsepState* hs = nullptr;
    // FastSpeech2 acoustic encoder
    dsd_encoder_config ecfg;
    std::vector<PackedGemm> g_qkv, g_oproj, g_ffn1, g_ffn2;
    std::vector<size_t> e_ln1g, e_ln1b, e_ln2g, e_ln2b;
    size_t e_lng = 0, e_lnb = 0, e_txt = 0, e_lang = SIZE_MAX, e_durw = 0, e_durb = 0, e_freqs = 0, e_spk = SIZE_MAX;
    size_t e_linw[7], e_linb[7];                     // pitch, energy, breathiness, voicing, tension, key shift, speed
    int eL = 0, eLs = 0, eB = 0, e_pos = 0;
    int e_ffn_act = DSD_FFN_GELU;                    // TransformerFFNLayer's activation (DSD_FFN_*)
    float *e_x = nullptr, *e_y = nullptr, *e_qkv = nullptr, *e_mid = nullptr, *e_nonpad = nullptr;
    int* e_dur = nullptr;
    DevBuf<float> e_arena;
    // token encoder (variance model): FastSpeech2Encoder + out_proj / DurationPredictor
    dsd_token_encoder_config tcfg;
    PackedGemm g_tout;
    std::vector<PackedGemm> g_dconv;
    std::vector<size_t> d_lng, d_lnb;
    size_t d_linw = 0, d_linb = 0;
    float *d_a = nullptr, *d_b = nullptr, *d_in = nullptr;
    int dC = 0;
    size_t freqs_off = 0;
    int emb_act = ACT_MISH;

    // workspace for (B, T)
    int B = 0, T = 0, Ts = 0;
    DevBuf<float> arena;
    size_t arena_floats = 0;
    float *cond_i = nullptr, *cp = nullptr, *xh = nullptr, *z = nullptr, *skip = nullptr, *hbuf = nullptr;
    float *xin = nullptr, *ubuf = nullptr, *vbuf = nullptr, *stats = nullptr, *lnpart = nullptr;
    float *io_in = nullptr, *io_out = nullptr;
    bool cond_ready = false;
    // ragged batches of the denoisers and the aux decoder (dsd_set_lengths): lengths and valid-tile lists; grid() == nullptr = dense
    RaggedOwner rag;
    // sampler state buffers
    DevBuf<float> state;
    int state_nbufs = 0;
    size_t state_buf_floats = 0;
    // step-embedding tables (columns = steps or batch items)
    DevBuf<float> emb_arena;
    int emb_cols = 0, Ns = 0;
    float *t_dev = nullptr, *E = nullptr, *Hd = nullptr, *E2 = nullptr, *D = nullptr;
    float* Dt = nullptr;            // D transposed: [step column][L * C rows] - what the layer kernels read their FiLM vectors from
    std::vector<float> t_host;

    std::map<std::string, GraphEntry> graphs;
    std::set<std::string> graph_seen;      // programs run once eagerly: a graph is captured when one comes back

    // timing of the layer kernels (dsd_kernel_timing): per kernel CLASS - a launch site of run_backbone and the variant of
    // it that ran (tile width, halo, segment of a mixed plan) - every timing_stride-th launch carries an event pair
    struct TimedClass {
        int key = 0;
        std::string name;           // the instantiation, as rocprofv3 prints it (filled in by the launcher that took the slot)
        double flops = 0, bytes = 0;    // algorithmic work of one launch (valid frames)
        long launches = 0;          // all launches of the class since timing was switched on
        std::vector<size_t> evs;    // indices into ev_pool
    };
    bool timing = false;
    std::vector<TimedClass> tclasses;
    long timing_evals = 0;         // backbone evaluations since timing was switched on
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> cal_pool;   // back-to-back pairs: the cost of the bracket itself
    size_t cal_used = 0;
    int timing_stride = 7;         // coprime with the layer count: every layer is sampled over a pass
};

namespace dsd {

inline bool is_wavenet(const dsd_handle* h) { return h->cfg.backbone == DSD_BACKBONE_WAVENET; }
inline bool is_aux(const dsd_handle* h) { return h->cfg.backbone == DSD_AUX_CONVNEXT; }
inline bool is_enc(const dsd_handle* h) { return h->cfg.backbone == DSD_ENC_FS2_ACOUSTIC; }
inline bool is_tok(const dsd_handle* h) { return h->cfg.backbone == DSD_ENC_FS2_TOKENS; }
inline bool is_voc(const dsd_handle* h) { return h->cfg.backbone == DSD_VOC_NSF_HIFIGAN; }
inline bool is_mel(const dsd_handle* h) { return h->cfg.backbone == DSD_MEL_ANALYSIS; }
inline bool is_pe(const dsd_handle* h) { return h->cfg.backbone == DSD_PE_RMVPE; }
inline bool is_hs(const dsd_handle* h) { return h->cfg.backbone == DSD_HNSEP_VR; }

// ------------------------------------------------------------------------------------------
// Which handle may call what.  Every exported call that takes a handle checks its own arguments for NULL and then calls
// enter() with the kinds it takes; nothing else decides whether a handle is of the right kind for a call (the is_*
// predicates above are for code that branches on the kind after entry).  INTEGRATION.md states the same sets as a table.
// ------------------------------------------------------------------------------------------
constexpr unsigned kind_bit(int backbone) { return 1u << backbone; }
constexpr unsigned K_WAVENET = kind_bit(DSD_BACKBONE_WAVENET), K_LYNXNET = kind_bit(DSD_BACKBONE_LYNXNET),
                   K_AUX = kind_bit(DSD_AUX_CONVNEXT), K_ENC = kind_bit(DSD_ENC_FS2_ACOUSTIC), K_VOC = kind_bit(DSD_VOC_NSF_HIFIGAN),
                   K_TOK = kind_bit(DSD_ENC_FS2_TOKENS), K_MEL = kind_bit(DSD_MEL_ANALYSIS), K_PE = kind_bit(DSD_PE_RMVPE),
                   K_HS = kind_bit(DSD_HNSEP_VR);
constexpr unsigned K_DENOISER = K_WAVENET | K_LYNXNET;
constexpr unsigned K_MODEL = K_DENOISER | K_AUX | K_ENC | K_VOC | K_TOK;         // all but the analysis kinds (mel, RMVPE, separator)
constexpr unsigned K_WEIGHTS = K_MODEL | K_PE | K_HS;                            // has a weight blob: a mel handle has none

// what a handle of each kind is, and the calls to use on it instead: the text of a wrong-kind refusal
struct KindName {
    const char *what, *use;
};
constexpr KindName kKindNames[] = {
    {"a WaveNet denoiser", "dsd_prepare_cond / dsd_denoise / dsd_sample"},
    {"a LYNXNet denoiser", "dsd_prepare_cond / dsd_denoise / dsd_sample"},
    {"an aux decoder", "dsd_aux_decode"},
    {"an acoustic encoder", "dsd_encode"},
    {"a vocoder", "dsd_vocode / dsd_vocode_ragged"},
    {"a token encoder", "dsd_token_encode / dsd_predict_dur"},
    {"a mel analysis handle", "dsd_mel_analyze"},
    {"an RMVPE pitch extractor", "dsd_rmvpe_infer / dsd_rmvpe_mel_to_hidden / dsd_rmvpe_decode*"},
    {"a harmonic-noise separator", "dsd_hnsep_separate / dsd_hnsep_mask / dsd_base_harmonic / dsd_variance_curves"},
};
static_assert(sizeof(kKindNames) / sizeof(kKindNames[0]) == DSD_HNSEP_VR + 1, "one name per DSD_* kind");

// path switches: every C-ABI entry point that launches kernels takes a snapshot into its handle (dsd_internal.h, PathOpts)
PathOpts read_path_opts();

enum : unsigned {
    ENTER_WEIGHTS = 1,      // the call reads the packed weights: dsd_finalize_weights must have succeeded
    ENTER_LAUNCH = 2,       // the call launches kernels: snapshot the path switches, make the handle's device current
};
// The one entry check (h != nullptr): DSD_ESTATE for a handle whose kind is not in `takes`, then for missing weights.
inline int enter(dsd_handle* h, const char* who, unsigned takes, unsigned flags = 0) {
    if (!(takes & kind_bit(h->cfg.backbone))) {
        const KindName& k = kKindNames[h->cfg.backbone];
        return fail(h, DSD_ESTATE, "%s: this handle is %s (use %s)", who, k.what, k.use);
    }
    if ((flags & ENTER_WEIGHTS) && !h->finalized) return fail(h, DSD_ESTATE, "%s: weights are not finalized", who);
    if (flags & ENTER_LAUNCH) {
        h->opts = read_path_opts();
        HIP_OK(h, hipSetDevice(h->cfg.device));
    }
    return DSD_OK;
}

// a state dict layout: the names a handle accepts, with their shapes
using ParamList = std::vector<std::pair<std::string, std::vector<int64_t>>>;

// every create function and dsd_cond_assemble: the device must exist before anything is placed on it
int select_device(const char* who, int device, bool say_range = true);
// What the seven create functions share, in this order: the arguments, struct_size, the family's own rules (`validate(cfg)`
// returns DSD_OK or the code of its fail()), the device ...
template <typename Cfg, typename Validate>
int create_check(const Cfg* cfg, dsd_handle** out, const char* who, Validate&& validate) {
    if (!cfg || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (cfg->struct_size != (int32_t)sizeof(Cfg))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, cfg->struct_size, sizeof(Cfg));
    if (int rc = validate(cfg)) return rc;
    return select_device(who, cfg->device);
}
// ... and the handle, its cfg zero but for the fields every kind has
inline dsd_handle* new_handle(int backbone, int device) {
    dsd_handle* h = new dsd_handle();
    memset(&h->cfg, 0, sizeof(h->cfg));
    h->cfg.struct_size = sizeof(dsd_config);
    h->cfg.backbone = backbone;
    h->cfg.device = device;
    return h;
}
// dsd_load_weight behind the caller's own name rules: looks `name` up in `expected` (nullptr: the caller has checked the
// shape itself), compares the shape and copies the host or device data into h->raw
int store_weight(dsd_handle* h, const ParamList* expected, const char* name, const float* data, const int64_t* shape,
                 int32_t ndim, int32_t on_device);
// dsd_finalize_weights: DSD_ESTATE naming every expected key that was not loaded
int check_missing(dsd_handle* h, const ParamList& expected);
// ... and its upload of the packed weights: a fresh allocation of host.size() + tail floats, the tail zeroed
int upload_blob(dsd_handle* h, DevBuf<float>& dev, const std::vector<float>& host, size_t tail);
// eval-mode BatchNorm (eps 1e-5) at state-dict prefix p as scale / shift, in double
void bn_scale_shift(const dsd_handle* h, const std::string& p, int C, std::vector<double>& sc, std::vector<double>& sh);
inline bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// What dsd_acoustic_spk_mix and dsd_variance_spk_mix share: every check on the host, then the ids into the object's own device
// block on the caller's stream and the one launch of spk_mix_kernels.hip.  `table` is nullptr for a model that has none to mix
// (`why_not` then says why: no use_spk_id, or a frozen_spk_embed).
struct SpkMixIds {
    std::vector<int> host;
    DevBuf<int> dev;
};
inline int spk_mix_run(const char* who, const dsd_spk_mix_args* g, const float* table, const char* why_not, int num_spk, int H,
                       int device, SpkMixIds& ids, void* stream) {
    if (!g) return fail(nullptr, DSD_EINVAL, "%s: NULL args", who);
    if (g->struct_size != (int32_t)sizeof(*g)) return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(*g));
    if (!table) return fail(nullptr, DSD_EINVAL, "%s: %s", who, why_not);
    if (!g->ids || !g->values || !g->out) return fail(nullptr, DSD_EINVAL, "%s: NULL ids, values or out", who);
    if (g->B < 1 || g->B > 65535) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, 65535]", who, g->B);
    if (g->rows < 1 || g->N < 1) return fail(nullptr, DSD_EINVAL, "%s: rows = %d and N = %d must be positive", who, g->rows, g->N);
    if ((int64_t)g->B * g->rows * std::max(g->N, H) > INT32_MAX || (int64_t)g->B * g->N > INT32_MAX)
        return fail(nullptr, DSD_EINVAL, "%s: [%d, %d, max(N = %d, H = %d)] holds more than 2^31 - 1 elements", who, g->B, g->rows, g->N, H);
    const size_t n = (size_t)g->B * g->N;
    for (size_t i = 0; i < n; ++i)
        if (g->ids[i] < 0 || g->ids[i] >= num_spk)
            return fail(nullptr, DSD_EINVAL, "%s: ids[%zu] = %d outside [0, num_spk = %d)", who, i, g->ids[i], num_spk);
    HIP_OK(nullptr, hipSetDevice(device));
    ids.host.assign(g->ids, g->ids + n);
    if (int rc = ids.dev.reserve(nullptr, n, who)) return rc;
    HIP_OK(nullptr, hipMemcpyAsync(ids.dev.p, ids.host.data(), n * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
    SpkMixP p;
    p.table = table; p.ids = ids.dev.p; p.values = g->values; p.out = g->out;
    p.rows = g->rows; p.N = g->N; p.H = H; p.normalize = g->normalize != 0; p.lanes = 0;
    const hipError_t e = launch_spk_mix(p, g->B, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return DSD_OK;
}

// mel analysis (mel_api.hip); RMVPE's front end runs it with a filterbank and geometry of its own
void mel_filterbank_host(const dsd_mel_config& c, std::vector<float>& w, bool htk = false);
bool mel_geometry(const dsd_mel_config& c, double keyshift, double speed, MelGeom& g);
int64_t mel_frames(const MelGeom& g, int64_t L);
int mel_state_build(MelState& mst, const dsd_mel_config* cfg, const std::vector<float>& w, const char* who);
int mel_run(dsd_handle* h, MelState& ms, const MelGeom& g, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
            const int64_t* lengths, float* mel_out, int64_t stride_b, int64_t stride_m, int64_t stride_t, void* stream,
            const char* who);
void mel_state_free(MelState* m);
// what dsd_load_weight, dsd_finalize_weights and dsd_destroy hand on to the family of the handle (rmvpe_api.hip, hnsep_api.hip)
int rmvpe_load_weight(dsd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim, int32_t on_device);
int rmvpe_finalize(dsd_handle* h);
void rmvpe_free(RmvpeState* r);
int hnsep_load_weight(dsd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim, int32_t on_device);
int hnsep_finalize(dsd_handle* h);
void hnsep_free(HnsepState* s);

}  // namespace dsd
