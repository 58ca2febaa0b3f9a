// libdsdenoise, host side of VR harmonic-noise separation and the variance curves: dsd_hnsep_*, dsd_base_harmonic,
// dsd_variance_curves (kernels: hnsep_kernels.hip)
#include "api_host.h"

// ------------------------------------------------------------------------------------------------------------------------------
// VR harmonic-noise separation and the variance curves (dsd_hnsep_*, dsd_base_harmonic, dsd_variance_curves):
// modules/hnsep/vr/ (nets.py, layers.py), utils/decomposed_waveform.py, utils/binarizer_utils.py
// ------------------------------------------------------------------------------------------------------------------------------
struct HsConvW {
    size_t w = 0, shift = 0;
    int cout = 0, cout_pad = 0, ks = 1, stride = 1, dil_f = 1, dil_t = 1, act = 0;
    std::vector<int> cin;                   // channels per source, in concat order
};
struct HsNetW {                             // one BaseNet
    int nin = 0, nout = 0, nin_lstm = 0, H = 0;
    HsConvW enc1, enc[4][2], aspp[5], bott, dec4, dec3, dec2, dec1, lconv, lproj, ldense;
    size_t whh = 0;
};
struct HsBasis {
    int N = 0, kind = 0;                    // kind 0: periodic Hann (VR), 1: Nuttall (_kth_harmonic)
    DevBuf<float> win, fwd, inv;
    int fRpad = 0, fKpad = 0, iRpad = 0, iKpad = 0;
};
struct HnsepState {
    dsd_hnsep_config cfg;
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected;
    DevBuf<float> blob;
    HsNetW net[5];                          // stg1 low, stg1 high, stg2 low, stg2 high, stg3 full
    HsConvW tail1, tail2, out;              // stg1_low_band_net.1, stg2_low_band_net.1, out
    std::vector<HsBasis> bases;
    DevBuf<float> ws;
    DevBuf<char> iws;                       // per-item counts and work lists
    std::vector<char> iw_host;
};

void dsd::hnsep_free(HnsepState* s) { delete s; }

namespace {

void hs_names_cba(std::vector<std::pair<std::string, std::vector<int64_t>>>& e, const std::string& p, int cin, int cout, int k) {
    e.push_back({p + ".conv.0.weight", {cout, cin, k, k}});
    for (const char* n : {"weight", "bias", "running_mean", "running_var"}) e.push_back({p + ".conv.1." + n, {cout}});
}

// BaseNet(nin, nout, nin_lstm, nout_lstm)  (nets.py:8-42)
void hs_names_net(std::vector<std::pair<std::string, std::vector<int64_t>>>& e, const std::string& p, int nin, int n,
                  int nin_lstm, int nout_lstm) {
    hs_names_cba(e, p + ".enc1", nin, n, 3);
    const int ch[5] = {1, 2, 4, 6, 8};
    for (int l = 1; l < 5; ++l) {
        hs_names_cba(e, p + ".enc" + std::to_string(l + 1) + ".conv1", n * ch[l - 1], n * ch[l], 3);
        hs_names_cba(e, p + ".enc" + std::to_string(l + 1) + ".conv2", n * ch[l], n * ch[l], 3);
    }
    hs_names_cba(e, p + ".aspp.conv1.1", 8 * n, 8 * n, 1);
    hs_names_cba(e, p + ".aspp.conv2", 8 * n, 8 * n, 1);
    for (int k = 3; k <= 5; ++k) hs_names_cba(e, p + ".aspp.conv" + std::to_string(k), 8 * n, 8 * n, 3);
    hs_names_cba(e, p + ".aspp.bottleneck", 40 * n, 8 * n, 1);
    hs_names_cba(e, p + ".dec4.conv1", 14 * n, 6 * n, 3);
    hs_names_cba(e, p + ".dec3.conv1", 10 * n, 4 * n, 3);
    hs_names_cba(e, p + ".dec2.conv1", 6 * n, 2 * n, 3);
    hs_names_cba(e, p + ".lstm_dec2.conv", 2 * n, 1, 1);
    const int H = nout_lstm / 2;
    for (const char* sfx : {"", "_reverse"}) {
        const std::string l = p + ".lstm_dec2.lstm.";
        e.push_back({l + "weight_ih_l0" + sfx, {4 * H, nin_lstm}});
        e.push_back({l + "weight_hh_l0" + sfx, {4 * H, H}});
        e.push_back({l + "bias_ih_l0" + sfx, {4 * H}});
        e.push_back({l + "bias_hh_l0" + sfx, {4 * H}});
    }
    e.push_back({p + ".lstm_dec2.dense.0.weight", {nin_lstm, nout_lstm}});
    e.push_back({p + ".lstm_dec2.dense.0.bias", {nin_lstm}});
    for (const char* nm : {"weight", "bias", "running_mean", "running_var"}) e.push_back({p + ".lstm_dec2.dense.1." + nm, {nin_lstm}});
    hs_names_cba(e, p + ".dec1.conv1", 3 * n + 1, n, 3);
}

const char* const HS_NET[5] = {"stg1_low_band_net.0", "stg1_high_band_net", "stg2_low_band_net.0", "stg2_high_band_net",
                               "stg3_full_band_net"};

struct HsNetDims {
    int nin, nout, nin_lstm, nout_lstm;
};
void hs_net_dims(const dsd_hnsep_config& c, HsNetDims d[5]) {
    const int nin = c.is_mono ? 2 : 4, nl = c.n_fft / 4, n = c.nout, L = c.nout_lstm;   // nin_lstm = max_bin / 2
    d[0] = {nin, n / 2, nl / 2, L};
    d[1] = {nin, n / 4, nl / 2, L / 2};
    d[2] = {n / 4 + nin, n, nl / 2, L};
    d[3] = {n / 4 + nin, n / 2, nl / 2, L / 2};
    d[4] = {3 * n / 4 + nin, n, nl, L};
}

std::vector<std::pair<std::string, std::vector<int64_t>>> hnsep_expected(const dsd_hnsep_config& c) {
    std::vector<std::pair<std::string, std::vector<int64_t>>> e;
    HsNetDims d[5];
    hs_net_dims(c, d);
    const int nin = c.is_mono ? 2 : 4, n = c.nout;
    for (int i = 0; i < 5; ++i) hs_names_net(e, HS_NET[i], d[i].nin, d[i].nout, d[i].nin_lstm, d[i].nout_lstm);
    hs_names_cba(e, "stg1_low_band_net.1", n / 2, n / 4, 1);
    hs_names_cba(e, "stg2_low_band_net.1", n, n / 2, 1);
    e.push_back({"out.weight", {nin, n, 1, 1}});
    e.push_back({"aux_out.weight", {nin, 3 * n / 4, 1, 1}});
    return e;
}

}  // namespace

int dsd::hnsep_load_weight(dsd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim, int32_t on_device) {
    if (!name) return fail(h, DSD_EINVAL, "dsd_load_weight: bad argument");
    const std::string n(name);
    if (ends_with(n, ".num_batches_tracked")) return DSD_OK;       // BatchNorm's step counter carries no value
    if (!data || !shape || ndim < 1 || ndim > 4) return fail(h, DSD_EINVAL, "dsd_load_weight: bad argument");
    HnsepState& r = *h->hs;
    const int rc = store_weight(h, &r.expected, name, data, shape, ndim, on_device);
    if (rc == DSD_OK) h->finalized = false;
    return rc;
}

namespace {

// w(co, ci, kf, kt) of a conv over the concat `cin` (sources in order) -> [(source, kf ks + kt, channel < Cp)][cout_pad],
// times sc[co]; shift -> [cout_pad]
template <typename W>
HsConvW hs_pack(std::vector<float>& blob, W&& w, int cout, std::vector<int> cin, int ks, const std::vector<double>& sc,
                const std::vector<double>& sh) {
    HsConvW c;
    c.cout = cout;
    c.cout_pad = (cout + 15) / 16 * 16;
    c.ks = ks;
    c.cin = cin;
    size_t rows = 0;
    for (int cs : cin) rows += (size_t)ks * ks * ((cs + 3) / 4 * 4);
    c.w = blob.size();
    blob.resize(blob.size() + rows * c.cout_pad, 0.f);
    size_t row = 0;
    int cb = 0;
    for (int cs : cin) {
        const int cp = (cs + 3) / 4 * 4;
        for (int kf = 0; kf < ks; ++kf)
            for (int kt = 0; kt < ks; ++kt) {
                for (int ci = 0; ci < cs; ++ci)
                    for (int co = 0; co < cout; ++co) blob[c.w + (row + ci) * c.cout_pad + co] = (float)(w(co, cb + ci, kf, kt) * sc[co]);
                row += cp;
            }
        cb += cs;
    }
    c.shift = blob.size();
    blob.resize(blob.size() + c.cout_pad, 0.f);
    for (int co = 0; co < cout; ++co) blob[c.shift + co] = (float)sh[co];
    return c;
}

// Conv2DBNActiv under `p` over the concat `cin`
HsConvW hs_pack_cba(const dsd_handle* h, std::vector<float>& blob, const std::string& p, int cout, std::vector<int> cin, int ks,
                    int stride, int dil_f, int dil_t, int act) {
    std::vector<double> sc, sh;
    bn_scale_shift(h, p + ".conv.1", cout, sc, sh);
    int ct = 0;
    for (int v : cin) ct += v;
    const std::vector<float>& W = h->raw.at(p + ".conv.0.weight").data;
    HsConvW c = hs_pack(blob, [&](int co, int ci, int kf, int kt) { return (double)W[(((size_t)co * ct + ci) * ks + kf) * ks + kt]; },
                        cout, cin, ks, sc, sh);
    c.stride = stride;
    c.dil_f = dil_f;
    c.dil_t = dil_t;
    c.act = act;
    return c;
}

void hs_pack_net(const dsd_handle* h, std::vector<float>& blob, HsNetW& N, const std::string& p, const HsNetDims& d,
                 const std::vector<int>& in_split) {
    const int n = d.nout;
    N.nin = d.nin;
    N.nout = n;
    N.nin_lstm = d.nin_lstm;
    N.H = d.nout_lstm / 2;
    N.enc1 = hs_pack_cba(h, blob, p + ".enc1", n, in_split, 3, 1, 1, 1, 1);
    const int ch[5] = {1, 2, 4, 6, 8};
    for (int l = 1; l < 5; ++l) {
        const std::string q = p + ".enc" + std::to_string(l + 1);
        N.enc[l - 1][0] = hs_pack_cba(h, blob, q + ".conv1", n * ch[l], {n * ch[l - 1]}, 3, 2, 1, 1, 2);
        N.enc[l - 1][1] = hs_pack_cba(h, blob, q + ".conv2", n * ch[l], {n * ch[l]}, 3, 1, 1, 1, 2);
    }
    N.aspp[0] = hs_pack_cba(h, blob, p + ".aspp.conv1.1", 8 * n, {8 * n}, 1, 1, 1, 1, 1);
    N.aspp[1] = hs_pack_cba(h, blob, p + ".aspp.conv2", 8 * n, {8 * n}, 1, 1, 1, 1, 1);
    const int dl[3][2] = {{4, 2}, {8, 4}, {12, 6}};      // BaseNet's dilations: (bins, frames)
    for (int k = 0; k < 3; ++k)
        N.aspp[2 + k] = hs_pack_cba(h, blob, p + ".aspp.conv" + std::to_string(k + 3), 8 * n, {8 * n}, 3, 1, dl[k][0], dl[k][1], 1);
    N.bott = hs_pack_cba(h, blob, p + ".aspp.bottleneck", 8 * n, {8 * n, 32 * n}, 1, 1, 1, 1, 1);
    N.dec4 = hs_pack_cba(h, blob, p + ".dec4.conv1", 6 * n, {8 * n, 6 * n}, 3, 1, 1, 1, 1);
    N.dec3 = hs_pack_cba(h, blob, p + ".dec3.conv1", 4 * n, {6 * n, 4 * n}, 3, 1, 1, 1, 1);
    N.dec2 = hs_pack_cba(h, blob, p + ".dec2.conv1", 2 * n, {4 * n, 2 * n}, 3, 1, 1, 1, 1);
    N.lconv = hs_pack_cba(h, blob, p + ".lstm_dec2.conv", 1, {2 * n}, 1, 1, 1, 1, 1);
    N.dec1 = hs_pack_cba(h, blob, p + ".dec1.conv1", n, {2 * n + 1, n}, 3, 1, 1, 1, 1);
    // the LSTM's input projection of both directions as one 1x1 conv over the bins: cout = 2 x 4H (forward | reverse),
    // shift = b_ih + b_hh
    const int H = N.H, G = 4 * H, K = d.nin_lstm;
    const std::string l = p + ".lstm_dec2.lstm.";
    const std::vector<float>& wf = h->raw.at(l + "weight_ih_l0").data;
    const std::vector<float>& wr = h->raw.at(l + "weight_ih_l0_reverse").data;
    std::vector<double> one(2 * G, 1.0), bias(2 * G);
    for (int d2 = 0; d2 < 2; ++d2) {
        const char* sfx = d2 ? "_reverse" : "";
        const auto &bi = h->raw.at(l + "bias_ih_l0" + sfx).data, &bh = h->raw.at(l + "bias_hh_l0" + sfx).data;
        for (int g = 0; g < G; ++g) bias[d2 * G + g] = (double)bi[g] + (double)bh[g];
    }
    N.lproj = hs_pack(blob, [&](int co, int ci, int, int) { return (double)(co < G ? wf[(size_t)co * K + ci] : wr[(size_t)(co - G) * K + ci]); },
                      2 * G, {K}, 1, one, bias);
    N.whh = blob.size();
    for (const char* sfx : {"", "_reverse"}) {
        const std::vector<float>& w = h->raw.at(l + "weight_hh_l0" + sfx).data;
        blob.insert(blob.end(), w.begin(), w.end());
    }
    // dense: Linear(2H, nin_lstm) + BatchNorm1d + ReLU folded: W s, (b - m) s + beta
    std::vector<double> sc, sh;
    bn_scale_shift(h, p + ".lstm_dec2.dense.1", K, sc, sh);
    const std::vector<float>& dw = h->raw.at(p + ".lstm_dec2.dense.0.weight").data;
    const std::vector<float>& db = h->raw.at(p + ".lstm_dec2.dense.0.bias").data;
    for (int k = 0; k < K; ++k) sh[k] += (double)db[k] * sc[k];
    N.ldense = hs_pack(blob, [&](int co, int ci, int, int) { return (double)dw[(size_t)co * 2 * H + ci]; }, K, {2 * H}, 1, sc, sh);
    N.ldense.act = 1;
}

}  // namespace

int dsd::hnsep_finalize(dsd_handle* h) {
    HnsepState& r = *h->hs;
    int rc = check_missing(h, r.expected);
    if (rc) return rc;
    const dsd_hnsep_config& c = r.cfg;
    const int C = c.is_mono ? 1 : 2, n = c.nout;
    HsNetDims d[5];
    hs_net_dims(c, d);
    std::vector<float> blob;
    // network input sources: re channels, im channels, then the stage outputs
    hs_pack_net(h, blob, r.net[0], HS_NET[0], d[0], {C, C});
    hs_pack_net(h, blob, r.net[1], HS_NET[1], d[1], {C, C});
    hs_pack_net(h, blob, r.net[2], HS_NET[2], d[2], {C, C, n / 4});
    hs_pack_net(h, blob, r.net[3], HS_NET[3], d[3], {C, C, n / 4});
    hs_pack_net(h, blob, r.net[4], HS_NET[4], d[4], {C, C, n / 4, n / 2});
    r.tail1 = hs_pack_cba(h, blob, "stg1_low_band_net.1", n / 4, {n / 2}, 1, 1, 1, 1, 1);
    r.tail2 = hs_pack_cba(h, blob, "stg2_low_band_net.1", n / 2, {n}, 1, 1, 1, 1, 1);
    const std::vector<float>& ow = h->raw.at("out.weight").data;
    std::vector<double> one(2 * C, 1.0), zero(2 * C, 0.0);
    r.out = hs_pack(blob, [&](int co, int ci, int, int) { return (double)ow[(size_t)co * n + ci]; }, 2 * C, {n}, 1, one, zero);
    HIP_OK(h, hipSetDevice(h->cfg.device));
    if ((rc = upload_blob(h, r.blob, blob, 0))) return rc;
    h->finalized = true;
    return DSD_OK;
}

namespace {

// the window (computed in double, stored as float32) and the forward / inverse DFT bases of one (N, kind), built on first use and
// complete before it returns (the cache serves every stream)
const HsBasis* hs_basis(dsd_handle* h, int N, int kind, hipStream_t st) {
    HnsepState& r = *h->hs;
    for (auto& b : r.bases)
        if (b.N == N && b.kind == kind) return &b;
    std::vector<float> w(N);
    for (int j = 0; j < N; ++j) {
        if (kind == 0) {       // torch.hann_window(N) (periodic)
            w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * j / N));
        } else {               // decomposed_waveform.py:168-174, in double and rounded once: the four terms cancel to 0 at the
                               // window's ends, where torch's float32 sum is 2.4e-7 off, and at hop == win / 2 the iSTFT
                               // divides by this window alone (3.2e-7 in the base harmonic at win 64, hop 32)
            const double ph = (double)j / (double)N * 2.0 * M_PI;
            w[j] = (float)(0.355768 - 0.487396 * cos(ph) + 0.144232 * cos(2.0 * ph) - 0.012604 * cos(3.0 * ph));
        }
    }
    HsBasis b;
    b.N = N;
    b.kind = kind;
    const int nb = N / 2 + 1;
    b.fRpad = (2 * nb + kDftRows - 1) / kDftRows * kDftRows;
    b.fKpad = N;
    b.iRpad = (N + kDftRows - 1) / kDftRows * kDftRows;
    b.iKpad = (2 * nb + kDftTaps - 1) / kDftTaps * kDftTaps;
    const char* who = "hs_basis";
    if (b.win.reserve(h, N, who) || b.fwd.reserve(h, (size_t)b.fRpad * b.fKpad, who) || b.inv.reserve(h, (size_t)b.iRpad * b.iKpad, who))
        return nullptr;
    if (hipMemcpy(b.win.p, w.data(), N * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        launch_hs_basis(b.fwd.p, b.win.p, b.fRpad, b.fKpad, nb, N, 0, st) != hipSuccess ||
        launch_hs_basis(b.inv.p, b.win.p, b.iRpad, b.iKpad, nb, N, 1, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)        // once per (N, window): later calls may come on other streams
        return nullptr;
    r.bases.push_back(std::move(b));
    return &r.bases.back();
}

// per-call host block of ints and longs uploaded once: `add()` appends an array at an 8-byte aligned offset and returns
// that offset, which the launches add to the block's device copy
struct HsUpload {
    std::vector<char>& buf;
    size_t add(const void* p, size_t n) {
        const size_t at = (buf.size() + 7) / 8 * 8;
        buf.resize(at + n);
        memcpy(buf.data() + at, p, n);
        return at;
    }
};

// CascadedNet.forward on B items of T_b frames (multiples of 16), input re / im sources at level 0 (bins [0, 2 bw)),
// mask written through `mv` (re at c cs, im at im_off + c cs) for all nb = n_fft / 2 + 1 bins
struct HsRun {
    dsd_handle* h;
    hipStream_t st;
    int B, Tal;
    const int* dT;                  // device: frames per item at level 0 .. 4 ([5][B])
    std::vector<int> Tl[5];         // host copy
    char* iw;                       // device work-list block
    std::vector<char>* iw_host;
    std::map<std::tuple<int, int, int>, std::pair<size_t, int>> conv_wl;   // (F, level out, level in) -> (offset, entries)
    bool dry = true;                // sizing pass: count the workspace, launch nothing
    float* ws = nullptr;            // bump allocator over the workspace
    size_t ws_used = 0, ws_peak = 0;
    float* alloc(size_t n) {
        float* p = dry ? nullptr : ws + ws_used;
        ws_used += (n + 63) / 64 * 64;
        ws_peak = std::max(ws_peak, ws_used);
        return p;
    }
};

HsSrc hs_src(const float* p, long bs, long fs, long ts, long cs, int C, int mode = 0) {
    HsSrc s;
    s.p = p;
    s.bs = bs;
    s.fs = fs;
    s.ts = ts;
    s.cs = cs;
    s.C = C;
    s.Cp = (C + 3) / 4 * 4;
    s.mode = mode;
    return s;
}
HsView hs_view(float* p, long bs, long fs, long ts, long cs) {
    HsView v;
    v.p = p;
    v.bs = bs;
    v.fs = fs;
    v.ts = ts;
    v.cs = cs;
    return v;
}
// a [B][F][Tal >> l][C] tensor
struct HsT {
    float* p = nullptr;
    int F = 0, T = 0, C = 0;
    long bs() const { return (long)F * T * C; }
    HsSrc src(int c0 = 0, int nc = -1, int mode = 0) const { return hs_src(p + c0, bs(), (long)T * C, C, 1, nc < 0 ? C - c0 : nc, mode); }
    HsView view(int f0 = 0, int c0 = 0) const { return hs_view(p + (long)f0 * T * C + c0, bs(), (long)T * C, C, 1); }
};

#define HS_LAUNCH(expr, what)                                                                            \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(h, DSD_EHIP, "%s launch failed: %s", what, hipGetErrorString(e_)); \
    } while (0)

// conv work lists (b, q0, T_l out, T_l in) over 64 positions for every (F >> l, level) a forward at bands Fb meets
void hs_conv_lists(HsRun& R, HsUpload& up, std::initializer_list<int> Fb) {
    auto add = [&](int F, int lo, int li) {
        const auto key = std::make_tuple(F, lo, li);
        if (R.conv_wl.count(key)) return;
        std::vector<int> e;
        for (int b = 0; b < R.B; ++b) {
            const int To = R.Tl[lo][b], Ti = R.Tl[li][b], np_ = F * To;
            for (int q0 = 0; q0 < np_; q0 += 64) e.insert(e.end(), {b, q0, To, Ti});
        }
        R.conv_wl[key] = {up.add(e.data(), e.size() * sizeof(int)), (int)(e.size() / 4)};
    };
    for (int l = 0; l < 5; ++l) {
        add(1, l, l);
        for (int F : Fb) {
            add(F >> l, l, l);
            if (l) add(F >> l, l, l - 1);
        }
    }
}

int hs_conv(HsRun& R, const HsConvW& cw, const std::vector<HsSrc>& srcs, HsView y, int F, int Fin, int lo, int li) {
    dsd_handle* h = R.h;
    if (R.dry) return DSD_OK;
    HsConvP p;
    memset(&p, 0, sizeof(p));
    p.nsrc = 0;
    for (const HsSrc& s : srcs) p.src[p.nsrc++] = s;
    if (p.nsrc != (int)cw.cin.size()) return fail(h, DSD_EINVAL, "internal: conv source count mismatch");
    for (int i = 0; i < p.nsrc; ++i)
        if (p.src[i].C != cw.cin[i]) return fail(h, DSD_EINVAL, "internal: conv source %d has %d channels, weights %d", i, p.src[i].C, cw.cin[i]);
    p.w = h->hs->blob.p + cw.w;
    p.shift = h->hs->blob.p + cw.shift;
    p.y = y;
    p.cout = cw.cout;
    p.cout_pad = cw.cout_pad;
    p.F = F;
    p.Fin = Fin;
    p.ks = cw.ks;
    p.stride = cw.stride;
    p.dil_f = cw.dil_f;
    p.dil_t = cw.dil_t;
    p.act = cw.act;
    const auto& wl = R.conv_wl.at(std::make_tuple(F, lo, li));
    p.work = (const int*)(R.iw + wl.first);
    HS_LAUNCH(launch_hs_conv(p, wl.second, R.st), "hnsep conv");
    return DSD_OK;
}

#define HS_RC(expr)             \
    do {                        \
        int rc_ = (expr);       \
        if (rc_) return rc_;    \
    } while (0)

// One BaseNet (nets.py:30-42) on the sources `in` (level 0, F bins) -> `out` (nout channels), in two phases around the
// LSTM recurrence, so that the sub-nets of one stage share its launch (hs_stage)
struct HsNetRun {
    const HsNetW* N;
    std::vector<HsSrc> in;
    int F;
    HsView out;
    HsT e0, d2;                     // kept for phase B: enc1's output (dec1's skip), dec2's output + the LSTM channel
    float *gi = nullptr, *ly = nullptr;
};

// phase A: encoders, ASPP, decoders down to dec2, the LSTM module's 1x1 conv and the input projection
int hs_net_a(HsRun& R, HsNetRun& r) {
    const HsNetW& N = *r.N;
    const int n = N.nout, B = R.B, F = r.F, ch[5] = {1, 2, 4, 6, 8};
    dsd_handle* h = R.h;
    auto T = [&](int l, int Fl, int C) {
        HsT t;
        t.F = Fl;
        t.T = R.Tal >> l;
        t.C = C;
        t.p = R.alloc((size_t)B * t.bs());
        return t;
    };
    HsT e[5];
    e[0] = T(0, F, n);
    HS_RC(hs_conv(R, N.enc1, r.in, e[0].view(), F, F, 0, 0));
    for (int l = 1; l < 5; ++l) {
        HsT a = T(l, F >> l, n * ch[l]);
        e[l] = T(l, F >> l, n * ch[l]);
        HS_RC(hs_conv(R, N.enc[l - 1][0], {e[l - 1].src()}, a.view(), F >> l, F >> (l - 1), l, l - 1));
        HS_RC(hs_conv(R, N.enc[l - 1][1], {a.src()}, e[l].view(), F >> l, F >> l, l, l));
    }
    // ASPP at level 4: the bin mean's 1x1 conv is broadcast over bins inside the bottleneck's staging
    const int F4 = F >> 4;
    HsT m = T(4, 1, 8 * n), f1 = T(4, 1, 8 * n), cat = T(4, F4, 32 * n), h4 = T(4, F4, 8 * n);
    if (!R.dry) {
        HsBinMeanP bp;
        bp.x = e[4].view();
        bp.y = m.view();
        bp.F = F4;
        bp.C = 8 * n;
        bp.T = R.dT + 4 * B;
        HS_LAUNCH(launch_hs_binmean(bp, B, R.Tal >> 4, R.st), "hnsep bin mean");
    }
    HS_RC(hs_conv(R, N.aspp[0], {m.src()}, f1.view(), 1, 1, 4, 4));
    for (int k = 1; k < 5; ++k) HS_RC(hs_conv(R, N.aspp[k], {e[4].src()}, cat.view(0, (k - 1) * 8 * n), F4, F4, 4, 4));
    HS_RC(hs_conv(R, N.bott, {f1.src(0, -1, 2), cat.src()}, h4.view(), F4, F4, 4, 4));
    // decoders: the x2 bilinear upsample of the coarser tensor is computed while the conv stages it
    HsT d4 = T(3, F >> 3, 6 * n), d3 = T(2, F >> 2, 4 * n);
    r.d2 = T(1, F >> 1, 2 * n + 1);
    HS_RC(hs_conv(R, N.dec4, {h4.src(0, -1, 1), e[3].src()}, d4.view(), F >> 3, F >> 3, 3, 3));
    HS_RC(hs_conv(R, N.dec3, {d4.src(0, -1, 1), e[2].src()}, d3.view(), F >> 2, F >> 2, 2, 2));
    HS_RC(hs_conv(R, N.dec2, {d3.src(0, -1, 1), e[1].src()}, r.d2.view(), F >> 1, F >> 1, 1, 1));
    // LSTMModule at level 1: 1x1 conv to one channel written as [t][bin], then the input projection of both directions
    const int F1 = F >> 1, T1 = R.Tal >> 1, H = N.H;
    float* li = R.alloc((size_t)B * T1 * F1);
    r.gi = R.alloc((size_t)B * T1 * 8 * H);
    r.ly = R.alloc((size_t)B * T1 * 2 * H);
    r.e0 = e[0];
    HS_RC(hs_conv(R, N.lconv, {r.d2.src(0, 2 * n)}, hs_view(li, (long)T1 * F1, 1, F1, 0), F1, F1, 1, 1));
    HS_RC(hs_conv(R, N.lproj, {hs_src(li, (long)T1 * F1, 0, F1, 1, F1)}, hs_view(r.gi, (long)T1 * 8 * H, 0, 8 * H, 1), 1, 1,
                  1, 1));
    return DSD_OK;
}

// phase B: the dense layer (BatchNorm1d folded) written as the extra channel 2n of d2, then dec1 -> out
int hs_net_b(HsRun& R, HsNetRun& r) {
    const HsNetW& N = *r.N;
    const int n = N.nout, T1 = R.Tal >> 1, H = N.H;
    HS_RC(hs_conv(R, N.ldense, {hs_src(r.ly, (long)T1 * 2 * H, 0, 2 * H, 1, 2 * H)},
                  hs_view(r.d2.p + 2 * n, r.d2.bs(), 0, r.d2.C, (long)r.d2.T * r.d2.C), 1, 1, 1, 1));
    HS_RC(hs_conv(R, N.dec1, {r.d2.src(0, -1, 1), r.e0.src()}, r.out, r.F, r.F, 0, 0));
    return DSD_OK;
}

// one stage of CascadedNet: phase A of each sub-net (1 or 2), ONE launch of the BiLSTM recurrence for all of them
// (a workgroup per item, sub-net and direction), phase B of each; the stage's scratch is released at the end
int hs_stage(HsRun& R, std::initializer_list<HsNetRun*> nets) {
    dsd_handle* h = R.h;
    const size_t mark = R.ws_used;
    for (HsNetRun* r : nets) HS_RC(hs_net_a(R, *r));
    if (!R.dry) {
        HsLstmP lp;
        memset(&lp, 0, sizeof(lp));
        int k = 0;
        for (HsNetRun* r : nets) {
            const int T1 = R.Tal >> 1, H = r->N->H;
            lp.net[k].gi = r->gi;
            lp.net[k].gi_bs = (long)T1 * 8 * H;
            lp.net[k].whh = h->hs->blob.p + r->N->whh;
            lp.net[k].y = r->ly;
            lp.net[k].y_bs = (long)T1 * 2 * H;
            lp.net[k].H = H;
            ++k;
        }
        lp.T = R.dT + R.B;
        HS_LAUNCH(launch_hs_lstm(lp, R.B, k, R.st), "hnsep lstm");
    }
    for (HsNetRun* r : nets) HS_RC(hs_net_b(R, *r));
    R.ws_used = mark;
    return DSD_OK;
}

// CascadedNet.forward (nets.py:99-133): re / im sources (C channels each, bins from 0) -> the bounded mask through `mv`
// (re at c cs, im at m_im + c cs) over n_fft / 2 + 1 bins
int hs_forward(HsRun& R, const HsSrc& xre, const HsSrc& xim, HsView mv, long m_im) {
    dsd_handle* h = R.h;
    HnsepState& S = *h->hs;
    const int C = S.cfg.is_mono ? 1 : 2, n = S.cfg.nout, mb = S.cfg.n_fft / 2, bw = mb / 2, B = R.B;
    auto T = [&](int Fl, int Ch) {
        HsT t;
        t.F = Fl;
        t.T = R.Tal;
        t.C = Ch;
        t.p = R.alloc((size_t)B * t.bs());
        return t;
    };
    HsT aux1 = T(mb, n / 4), aux2 = T(mb, n / 2), tl = T(bw, n), f3 = T(mb, n), o = T(mb, 2 * C);
    auto hi = [&](HsSrc s) {
        s.p += (long)bw * s.fs;
        return s;
    };
    auto part = [&](const HsT& t, int f0) {         // the bins from f0 of a full-band stage output
        HsSrc s = t.src();
        s.p += (long)f0 * s.fs;
        return s;
    };
    // stage 1: low and high band side by side (the low band's output through its 1x1 tail into aux1's low bins)
    HsT l1 = T(bw, n / 2);
    HsNetRun s1l{&S.net[0], {xre, xim}, bw, l1.view()}, s1h{&S.net[1], {hi(xre), hi(xim)}, bw, aux1.view(bw)};
    HS_RC(hs_stage(R, {&s1l, &s1h}));
    HS_RC(hs_conv(R, S.tail1, {l1.src()}, aux1.view(0), bw, bw, 0, 0));
    // stage 2: each band with its stage-1 output concatenated
    HsNetRun s2l{&S.net[2], {xre, xim, part(aux1, 0)}, bw, tl.view()}, s2h{&S.net[3], {hi(xre), hi(xim), part(aux1, bw)}, bw,
                                                                          aux2.view(bw)};
    HS_RC(hs_stage(R, {&s2l, &s2h}));
    HS_RC(hs_conv(R, S.tail2, {tl.src()}, aux2.view(0), bw, bw, 0, 0));
    // stage 3: the full band with both stages' outputs
    HsNetRun s3{&S.net[4], {xre, xim, aux1.src(), aux2.src()}, mb, f3.view()};
    HS_RC(hs_stage(R, {&s3}));
    HS_RC(hs_conv(R, S.out, {f3.src()}, o.view(), mb, mb, 0, 0));
    if (!R.dry) {
        HsMaskP mp;
        mp.x = o.view();
        mp.y = mv;
        mp.y_im = m_im;
        mp.F = mb + 1;
        mp.Fx = mb;
        mp.C = C;
        mp.T = R.dT;
        HS_LAUNCH(launch_hs_mask(mp, B, R.Tal, R.st), "hnsep mask");
    }
    return DSD_OK;
}

// set up R for B items of Tp[b] frames (multiples of 16): per-level frame counts, conv work lists
void hs_setup(HsRun& R, dsd_handle* h, HsUpload& up, const std::vector<int>& Tp, hipStream_t st, size_t& dT_off) {
    R.h = h;
    R.st = st;
    R.B = (int)Tp.size();
    R.Tal = 0;
    for (int v : Tp) R.Tal = std::max(R.Tal, v);
    std::vector<int> all;
    for (int l = 0; l < 5; ++l) {
        R.Tl[l].resize(R.B);
        for (int b = 0; b < R.B; ++b) all.push_back(R.Tl[l][b] = Tp[b] >> l);
    }
    dT_off = up.add(all.data(), all.size() * sizeof(int));
    const int mb = h->hs->cfg.n_fft / 2;
    hs_conv_lists(R, up, {mb / 2, mb});
}

// upload the host block, size the workspace by a dry run of `body`, then run it
template <typename Body>
int hs_execute(HsRun& R, std::vector<char>& up, size_t dT_off, const char* who, Body&& body) {
    dsd_handle* h = R.h;
    HnsepState& S = *h->hs;
    R.dry = true;
    R.ws_used = R.ws_peak = 0;
    HS_RC(body());
    const size_t need = R.ws_peak;
    if (need * 4 >= ((size_t)1 << 40)) return fail(h, DSD_EINVAL, "%s: batch too large for one call", who);
    HS_RC(S.ws.reserve(h, need, who));
    HS_RC(S.iws.reserve(h, std::max<size_t>(up.size(), 8), who));
    HIP_OK(h, hipMemcpyAsync(S.iws.p, up.data(), up.size(), hipMemcpyHostToDevice, R.st));
    R.iw = S.iws.p;
    R.dT = (const int*)(R.iw + dT_off);
    R.dry = false;
    R.ws = S.ws.p;
    R.ws_used = 0;
    return body();
}

// The STFT -> (mask) -> iSTFT -> overlap-add chain of dsd_hnsep_separate and dsd_base_harmonic.  The spectrum (and the
// network's mask) is an HsT [b][bin][t][re of the C channels | im of the C channels]; the frames are [(b C + c)][t < T][N].
struct HsDft {
    dsd_handle* h;
    hipStream_t st;
    const HsBasis* bs;
    std::string fam;                // "hnsep" / "base harmonic": the family in the launch error texts
    int hop, B;
    long Lmax;
    size_t fw = 0, iw = 0, len = 0, off0 = 0;      // offsets in the uploaded block: work lists, samples and offset per item
    int nfw = 0, niw = 0;
};

// the work lists (b, t0, L, T_b, channel, padL) per (item, 64-frame tile, channel): forward over fch channels with padL =
// off0[b] (the padded position of sample 0), inverse over C channels; and the overlap-add's per-item L and off0
void hs_dft_lists(HsDft& d, HsUpload& up, const std::vector<int>& Tp, const std::vector<int64_t>& L, const std::vector<int64_t>& off0,
                  int fch, int C) {
    std::vector<int> fw, iw;
    for (int b = 0; b < d.B; ++b)
        for (int t0 = 0; t0 < Tp[b]; t0 += kDftFrames) {
            for (int c = 0; c < fch; ++c) fw.insert(fw.end(), {b, t0, (int)L[b], Tp[b], c, (int)off0[b]});
            for (int c = 0; c < C; ++c) iw.insert(iw.end(), {b, t0, (int)L[b], Tp[b], c, 0});
        }
    d.nfw = (int)(fw.size() / 6);
    d.niw = (int)(iw.size() / 6);
    d.fw = up.add(fw.data(), fw.size() * 4);
    d.iw = up.add(iw.data(), iw.size() * 4);
    d.len = up.add(L.data(), d.B * 8);
    d.off0 = up.add(off0.data(), d.B * 8);
}

// blk: the device copy of the uploaded block
int hs_stft(const HsDft& d, const char* blk, const float* wav, long wav_sb, long wav_sc, bool reflect, const HsT& spec, int nrep) {
    dsd_handle* h = d.h;
    HsStftP p;
    p.basis = d.bs->fwd.p;
    p.N = d.bs->N;
    p.nb = spec.F;
    p.wav = wav;
    p.wav_sb = wav_sb;
    p.wav_sc = wav_sc;
    p.H = d.hop;
    p.reflect = reflect ? 1 : 0;
    p.spec = spec.p;
    p.s_sb = spec.bs();
    p.s_sf = (long)spec.T * spec.C;
    p.s_st = spec.C;
    p.s_cim = spec.C / 2;
    p.nrep = nrep;
    p.work = (const int*)(blk + d.fw);
    HS_LAUNCH(launch_hs_stft(p, d.nfw, d.bs->fRpad / kDftRows, d.st), (d.fam + " stft").c_str());
    return DSD_OK;
}

// spectrum x mask -> frames -> out.  mask: the network's, or NULL for the f0 bin mask of f0[b f0_sb + t], f0_len[b] frames,
// at sample rate sr.  T: frames per item (device); o_sc 0: the channels' mean
int hs_istft_ola(const HsDft& d, const char* blk, const HsT& spec, const HsT* mask, const float* f0, long f0_sb, const int* f0_len,
                 float sr, float* frames, const int* T, float* out, long o_sb, long o_sc) {
    dsd_handle* h = d.h;
    const int N = d.bs->N, C = spec.C / 2;
    HsIstftP p = {};                // (the mask's strides stay 0 under the f0 bin mask)
    p.basis = d.bs->inv.p;
    p.Kpad = d.bs->iKpad;
    p.N = N;
    p.nb = spec.F;
    p.spec = spec.p;
    p.s_sb = spec.bs();
    p.s_sf = (long)spec.T * spec.C;
    p.s_st = spec.C;
    p.s_cim = C;
    p.mask = mask ? mask->p : nullptr;
    if (mask) {
        p.m_sb = mask->bs();
        p.m_sf = (long)mask->T * mask->C;
        p.m_st = mask->C;
        p.m_cim = mask->C / 2;
        p.mask_F = mask->F;
    }
    p.f0 = f0;
    p.f0_sb = f0_sb;
    p.f0_len = f0_len;
    p.sr = sr;
    p.half_width = 3.5f;
    p.frames = frames;
    p.f_sb = (long)spec.T * N;
    p.nch = C;
    p.work = (const int*)(blk + d.iw);
    HS_LAUNCH(launch_hs_istft(p, d.niw, d.bs->iRpad / kDftRows, d.st), (d.fam + " istft").c_str());
    HsOlaP op;
    op.frames = frames;
    op.f_sb = p.f_sb;
    op.win = d.bs->win.p;
    op.N = N;
    op.H = d.hop;
    op.nch = C;
    op.T = T;
    op.len = (const long*)(blk + d.len);
    op.off0 = (const long*)(blk + d.off0);
    op.out = out;
    op.o_sb = o_sb;
    op.o_sc = o_sc;
    HS_LAUNCH(launch_hs_ola(op, d.B, d.Lmax, d.st), (d.fam + " overlap-add").c_str());
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_hnsep_create(const dsd_hnsep_config* cfg, dsd_handle** out) {
    const int rc = create_check(cfg, out, "dsd_hnsep_create", [](const dsd_hnsep_config* c) {
        if (c->n_fft < 128 || c->n_fft > 4096 || c->n_fft % 64 != 0 || c->hop_length < 1 || c->hop_length > c->n_fft / 2 ||
            c->nout < 4 || c->nout > 64 || c->nout % 4 != 0 || c->nout_lstm < 8 || c->nout_lstm > 128 || c->nout_lstm % 8 != 0 ||
            (c->is_mono != 0 && c->is_mono != 1))
            return fail(nullptr, DSD_EINVAL, "dsd_hnsep_create: need n_fft a multiple of 64 in [128, 4096], 1 <= hop_length <= "
                        "n_fft / 2, nout a multiple of 4 in [4, 64], nout_lstm a multiple of 8 in [8, 128], is_mono 0 or 1");
        return DSD_OK;
    });
    if (rc) return rc;
    dsd_handle* h = new_handle(DSD_HNSEP_VR, cfg->device);
    h->cfg.in_dims = cfg->n_fft / 2 + 1;
    h->cfg.n_feats = 1;
    h->hs = new HnsepState();
    h->hs->cfg = *cfg;
    h->hs->expected = hnsep_expected(*cfg);
    *out = h;
    return DSD_OK;
}

int64_t dsd_hnsep_num_frames(int64_t n_samples, int32_t hop_length) {
    if (n_samples < 1 || hop_length < 1) return fail(nullptr, DSD_EINVAL, "dsd_hnsep_num_frames: need n_samples, hop_length >= 1");
    const int64_t n = n_samples / hop_length + 1;
    return 32 * (n / 32 + 1);
}

int dsd_hnsep_mask(dsd_handle* h, const float* spec, int32_t B, int32_t T, int64_t s_stride_b, int64_t s_stride_c,
                   int64_t s_stride_f, int64_t s_stride_t, const int64_t* lengths, float* mask_out, int64_t m_stride_b,
                   int64_t m_stride_c, int64_t m_stride_f, int64_t m_stride_t, void* stream) {
    const char* who = "dsd_hnsep_mask";
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: null handle", who);
    HS_RC(enter(h, who, K_HS, ENTER_WEIGHTS | ENTER_LAUNCH));
    if (!spec || !mask_out || B < 1 || T < 16) return fail(h, DSD_EINVAL, "%s: bad argument", who);
    std::vector<int> Tp(B);
    for (int b = 0; b < B; ++b) {
        const int64_t v = lengths ? lengths[b] : T;
        if (v < 16 || v > T || v % 16 != 0)
            return fail(h, DSD_EINVAL, "%s: frame count %lld of item %d is not a multiple of 16 in [16, T]", who, (long long)v, b);
        Tp[b] = (int)v;
    }
    HnsepState& S = *h->hs;
    const int C = S.cfg.is_mono ? 1 : 2;
    hipStream_t st = (hipStream_t)stream;
    S.iw_host.clear();
    HsUpload up{S.iw_host};
    HsRun R;
    size_t dT_off = 0;
    hs_setup(R, h, up, Tp, st, dT_off);
    const HsSrc xre = hs_src(spec, (long)s_stride_b, (long)s_stride_f, (long)s_stride_t, (long)s_stride_c, C);
    const HsSrc xim = hs_src(spec + 1, (long)s_stride_b, (long)s_stride_f, (long)s_stride_t, (long)s_stride_c, C);
    const HsView mv = hs_view(mask_out, (long)m_stride_b, (long)m_stride_f, (long)m_stride_t, (long)m_stride_c);
    return hs_execute(R, S.iw_host, dT_off, who, [&]() { return hs_forward(R, xre, xim, mv, 1); });
}

int dsd_hnsep_separate(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                       int64_t wav_stride_c, const int64_t* lengths, float* harmonic_out, int64_t out_stride_b,
                       int64_t out_stride_c, void* stream) {
    const char* who = "dsd_hnsep_separate";
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: null handle", who);
    HS_RC(enter(h, who, K_HS, ENTER_WEIGHTS | ENTER_LAUNCH));
    if (!wav || !harmonic_out || B < 1 || n_samples < 1 || wav_stride_c < 0 || out_stride_c < 0)
        return fail(h, DSD_EINVAL, "%s: bad argument", who);
    HnsepState& S = *h->hs;
    const int N = S.cfg.n_fft, hop = S.cfg.hop_length, C = S.cfg.is_mono ? 1 : 2, nb = N / 2 + 1;
    const bool repeat = C == 1 || wav_stride_c == 0;     // one clip on every channel: one STFT, copied to the channels
    std::vector<int> Tp(B);
    std::vector<int64_t> L(B), off0(B);
    int64_t Lmax = 0;
    for (int b = 0; b < B; ++b) {
        L[b] = lengths ? lengths[b] : n_samples;
        if (L[b] < 1 || L[b] > n_samples) return fail(h, DSD_EINVAL, "%s: length %lld of item %d out of [1, n_samples]", who, (long long)L[b], b);
        if (L[b] >= ((int64_t)1 << 30)) return fail(h, DSD_EINVAL, "%s: clip too long", who);
        const int64_t nf = L[b] / hop + 1, Tpad = (32 * (nf / 32 + 1) - 1) * hop - L[b], Tl_pad = Tpad / 2 / hop * hop;
        Tp[b] = (int)(32 * (nf / 32 + 1));
        off0[b] = N / 2 + Tl_pad;       // padded position of sample 0 in the iSTFT's frame space
        Lmax = std::max(Lmax, L[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    const HsBasis* bs = hs_basis(h, N, 0, st);
    if (!bs) return fail(h, DSD_ENOMEM, "%s: the DFT bases could not be placed on the device", who);
    S.iw_host.clear();
    HsUpload up{S.iw_host};
    HsRun R;
    size_t dT_off = 0;
    hs_setup(R, h, up, Tp, st, dT_off);
    HsDft d{h, st, bs, "hnsep", hop, B, (long)Lmax};
    hs_dft_lists(d, up, Tp, L, off0, repeat ? 1 : C, C);
    const int Tal = R.Tal;
    return hs_execute(R, S.iw_host, dT_off, who, [&]() -> int {
        HsT spec, mask;
        spec.F = mask.F = nb;
        spec.T = mask.T = Tal;
        spec.C = mask.C = 2 * C;
        spec.p = R.alloc((size_t)B * spec.bs());
        mask.p = R.alloc((size_t)B * mask.bs());
        float* frames = R.alloc((size_t)B * C * Tal * N);
        if (!R.dry) HS_RC(hs_stft(d, R.iw, wav, (long)wav_stride_b, repeat ? 0 : (long)wav_stride_c, false, spec, repeat ? C : 1));
        HS_RC(hs_forward(R, spec.src(0, C), spec.src(C, C), mask.view(), C));
        if (R.dry) return DSD_OK;
        return hs_istft_ola(d, R.iw, spec, &mask, nullptr, 0, nullptr, 0.f, frames, R.dT, harmonic_out, (long)out_stride_b,
                            C == 1 ? 0 : (long)out_stride_c);
    });
}

int dsd_base_harmonic(dsd_handle* h, const float* harmonic, int32_t B, int64_t n_samples, int64_t stride_b,
                      const int64_t* lengths, const float* f0, int64_t f0_stride_b, const int64_t* f0_lengths,
                      int32_t sample_rate, int32_t hop_size, int32_t win_size, float* out, int64_t out_stride_b,
                      void* stream) {
    const char* who = "dsd_base_harmonic";
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: null handle", who);
    HS_RC(enter(h, who, K_HS, ENTER_LAUNCH));       // no weights are used
    if (!harmonic || !f0 || !f0_lengths || !out || B < 1 || n_samples < 1 || sample_rate < 1 || win_size < 64 ||
        win_size > 4096 || win_size % 32 != 0 || hop_size < 1 || hop_size > win_size / 2)
        return fail(h, DSD_EINVAL, "%s: bad argument (win_size must be a multiple of 32 in [64, 4096], 1 <= hop_size <= "
                    "win_size / 2: past that the Nuttall window's square sum reaches 0, where torch.istft raises)", who);
    HnsepState& S = *h->hs;
    const int N = win_size, nb = N / 2 + 1;
    std::vector<int> Tp(B), f0n(B);
    std::vector<int64_t> L(B), off0(B, N / 2);
    int64_t Lmax = 0;
    int Tal = 0;
    for (int b = 0; b < B; ++b) {
        L[b] = lengths ? lengths[b] : n_samples;
        if (L[b] <= N / 2 || L[b] > n_samples || L[b] >= ((int64_t)1 << 30))
            return fail(h, DSD_EINVAL, "%s: length %lld of item %d must exceed win_size / 2 (torch's reflect pad)", who, (long long)L[b], b);
        Tp[b] = (int)(L[b] / hop_size + 1);
        if (f0_lengths[b] < 0) return fail(h, DSD_EINVAL, "%s: negative f0 length", who);
        f0n[b] = (int)std::min<int64_t>(f0_lengths[b], Tp[b]);
        Lmax = std::max(Lmax, L[b]);
        Tal = std::max(Tal, Tp[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    const HsBasis* bs = hs_basis(h, N, 1, st);
    if (!bs) return fail(h, DSD_ENOMEM, "%s: the DFT bases could not be placed on the device", who);
    S.iw_host.clear();
    HsUpload up{S.iw_host};
    const size_t T_off = up.add(Tp.data(), B * 4), f0n_off = up.add(f0n.data(), B * 4);
    HsDft d{h, st, bs, "base harmonic", hop_size, B, (long)Lmax};
    hs_dft_lists(d, up, Tp, L, off0, 1, 1);
    HsT spec;
    spec.F = nb;
    spec.T = Tal;
    spec.C = 2;
    HS_RC(S.ws.reserve(h, (size_t)B * spec.bs() + (size_t)B * Tal * N, who));
    HS_RC(S.iws.reserve(h, up.buf.size(), who));
    const char* iws = S.iws.p;
    HIP_OK(h, hipMemcpyAsync(S.iws.p, S.iw_host.data(), S.iw_host.size(), hipMemcpyHostToDevice, st));
    spec.p = S.ws.p;
    HS_RC(hs_stft(d, iws, harmonic, (long)stride_b, 0, true, spec, 1));
    return hs_istft_ola(d, iws, spec, nullptr, f0, (long)f0_stride_b, (const int*)(iws + f0n_off), (float)sample_rate,
                        S.ws.p + (size_t)B * spec.bs(), (const int*)(iws + T_off), out, (long)out_stride_b, 0);
}

int dsd_variance_curves(dsd_handle* h, const float* wav, const float* harmonic, const float* base, int32_t B,
                        int64_t stride_b, const int64_t* lengths, int32_t hop_size, int32_t win_size, const int64_t* frames,
                        int32_t tension_domain, int32_t energy_db, float* energy, float* breathiness, float* voicing,
                        float* tension, int64_t out_stride_b, void* stream) {
    const char* who = "dsd_variance_curves";
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: null handle", who);
    HS_RC(enter(h, who, K_HS, ENTER_LAUNCH));       // no weights are used
    if (B < 1 || !lengths || !frames || hop_size < 1 || win_size < 1 || tension_domain < 0 || tension_domain > 2)
        return fail(h, DSD_EINVAL, "%s: bad argument", who);
    if ((energy && !wav) || (breathiness && (!wav || !harmonic)) || (voicing && !harmonic) || (tension && (!harmonic || !base)))
        return fail(h, DSD_EINVAL, "%s: a requested curve is missing its input signal", who);
    HnsepState& S = *h->hs;
    std::vector<int> nfr(B), len(B);
    std::vector<int64_t> L(B);
    int Tmax = 1;
    for (int b = 0; b < B; ++b) {
        L[b] = lengths[b];
        if (L[b] < 1 || L[b] >= ((int64_t)1 << 30) || frames[b] < 0 || frames[b] >= ((int64_t)1 << 24))
            return fail(h, DSD_EINVAL, "%s: bad length of item %d", who, b);
        const int64_t Lp = L[b] + 2 * (win_size / 2);
        nfr[b] = Lp < win_size ? 0 : (int)(1 + (Lp - win_size) / hop_size);     // librosa.util.frame
        len[b] = (int)frames[b];
        Tmax = std::max(Tmax, nfr[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    S.iw_host.clear();
    HsUpload up{S.iw_host};
    const size_t n_off = up.add(nfr.data(), B * 4), l_off = up.add(len.data(), B * 4), L_off = up.add(L.data(), B * 8);
    HS_RC(S.ws.reserve(h, (size_t)4 * B * Tmax, who));
    HS_RC(S.iws.reserve(h, up.buf.size(), who));
    const char* iws = S.iws.p;
    HIP_OK(h, hipMemcpyAsync(S.iws.p, S.iw_host.data(), S.iw_host.size(), hipMemcpyHostToDevice, st));
    HsRmsP rp;
    rp.wav = (energy || breathiness) ? wav : nullptr;
    rp.harm = (breathiness || voicing || tension) ? harmonic : nullptr;
    rp.base = tension ? base : nullptr;
    rp.sb = (long)stride_b;
    rp.len = (const long*)(iws + L_off);
    rp.nfr = (const int*)(iws + n_off);
    rp.hop = hop_size;
    rp.win = win_size;
    rp.B = B;
    rp.Tmax = Tmax;
    rp.rms = S.ws.p;
    HS_LAUNCH(launch_hs_rms(rp, st), "variance rms");
    HsCurvesP cp;
    cp.rms = S.ws.p;
    cp.nfr = rp.nfr;
    cp.length = (const int*)(iws + l_off);
    cp.B = B;
    cp.Tmax = Tmax;
    cp.domain = tension_domain;
    cp.db = energy_db ? 1 : 0;
    cp.out[0] = energy;
    cp.out[1] = breathiness;
    cp.out[2] = voicing;
    cp.out[3] = tension;
    cp.o_sb = (long)out_stride_b;
    HS_LAUNCH(launch_hs_curves(cp, st), "variance curves");
    return DSD_OK;
}

}  // extern "C"
