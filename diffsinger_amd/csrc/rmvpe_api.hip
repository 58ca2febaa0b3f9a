// libdsdenoise, host side of RMVPE pitch extraction: dsd_rmvpe_* (kernels: rmvpe_kernels.hip; front end: mel_api.hip)
#include "api_host.h"
#include <float.h>

// ------------------------------------------------------------------------------------------------------------------------------
// RMVPE pitch extraction (dsd_rmvpe_*): modules/pe/rmvpe/ (inference.py, model.py, deepunet.py, seq.py, spec.py, utils.py)
// ------------------------------------------------------------------------------------------------------------------------------
// dsd_rmvpe_*: the offsets of a conv's packed parts in the weight blob (floats)
struct RmConvW {
    size_t w = 0, shift = 0, ws = 0, bs = 0;
    int cin = 0, cout = 0, cout_pad = 0;
    bool sc = false;            // a 1x1 shortcut conv (ws / bs): ConvBlockRes with in != out
};
struct RmBlockW {
    RmConvW c1, c2;             // c2 carries the residual
};
struct RmvpeState {
    dsd_rmvpe_config cfg;
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected;
    DevBuf<float> blob;
    float bn0_scale = 1.f, bn0_shift = 0.f;                  // unet.encoder.bn (1 channel)
    std::vector<std::vector<RmBlockW>> enc, inter, dec;     // [layer][block]
    std::vector<RmConvW> up;                                 // decoder ConvTranspose2d per layer
    RmConvW head;                                            // cnn
    size_t wih = 0, bih = 0, whh = 0, bhh = 0, fcw = 0, fcb = 0;
    MelState* mel = nullptr;                                 // MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)
    struct Resampler {
        int sr = 0, orig = 0, nw = 0, width = 0, K = 0;
        DevBuf<float> dev;
    };
    std::vector<Resampler> rs;                               // per input sample rate met so far
    DevBuf<float> ws;                                        // workspace
    DevBuf<int> iws;                                         // per-item counts and work lists
    std::vector<int> iw_host, lens_host;
    DevBuf<float> fe;                                        // front end: log-mel, resampled audio
    DevBuf<int> lens;                                        // resampler: samples in / out per item
    // Viterbi decode: the transition table (built at the first call), log_prob, the back-pointers, frame counts + the path
    DevBuf<double> vt_tab, vt_lp;
    DevBuf<unsigned short> vt_ptr;
    DevBuf<int> vt_iw;
    std::vector<int> vt_iw_host;
};

namespace {

constexpr int RM_MELS = 128, RM_CLASSES = 360, RM_HOP = 160, RM_NFFT = 1024;

dsd_mel_config rmvpe_mel_config(int device) {
    dsd_mel_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(dsd_mel_config);
    c.sampling_rate = 16000;
    c.n_fft = RM_NFFT;
    c.win_size = RM_NFFT;
    c.hop_size = RM_HOP;
    c.num_mels = RM_MELS;
    c.fmin = 30.0;
    c.fmax = 8000.0;
    c.clip_val = 1e-5;
    c.device = device;
    return c;
}

// torch.stft(center=True): reflect pads n_fft / 2 on both sides, T = 1 + L // 160
MelGeom rmvpe_geometry() {
    MelGeom g;
    g.N = g.W = RM_NFFT;
    g.H = RM_HOP;
    g.off = 0;
    g.padL = g.padR = RM_NFFT / 2;
    g.rescale = false;
    return g;
}

int64_t rmvpe_resampled_length(int64_t L, int sr) {
    if (sr == 16000) return L;
    const int g = std::gcd(sr, 16000), orig = sr / g, nw = 16000 / g;
    return ((int64_t)nw * L + orig - 1) / orig;       // ceil(new L / orig)
}

// ConvBlockRes(cin, cout) under `prefix`: conv.0 / conv.3 (3x3, no bias), conv.1 / conv.4 (BatchNorm2d), shortcut when cin != cout
void rmvpe_block_names(std::vector<std::pair<std::string, std::vector<int64_t>>>& e, const std::string& prefix, int cin, int cout) {
    const char* bn[4] = {"weight", "bias", "running_mean", "running_var"};
    e.push_back({prefix + ".conv.0.weight", {cout, cin, 3, 3}});
    for (auto n : bn) e.push_back({prefix + ".conv.1." + n, {cout}});
    e.push_back({prefix + ".conv.3.weight", {cout, cout, 3, 3}});
    for (auto n : bn) e.push_back({prefix + ".conv.4." + n, {cout}});
    if (cin != cout) {
        e.push_back({prefix + ".shortcut.weight", {cout, cin, 1, 1}});
        e.push_back({prefix + ".shortcut.bias", {cout}});
    }
}

std::vector<std::pair<std::string, std::vector<int64_t>>> rmvpe_expected(const dsd_rmvpe_config& c) {
    std::vector<std::pair<std::string, std::vector<int64_t>>> e;
    const char* bn[4] = {"weight", "bias", "running_mean", "running_var"};
    const int E = c.en_de_layers, C = c.en_out_channels, nb = c.n_blocks;
    for (auto n : bn) e.push_back({std::string("unet.encoder.bn.") + n, {1}});
    for (int l = 0; l < E; ++l) {
        const int cin = l == 0 ? 1 : C << (l - 1), cout = C << l;
        for (int k = 0; k < nb; ++k)
            rmvpe_block_names(e, "unet.encoder.layers." + std::to_string(l) + ".conv." + std::to_string(k), k ? cout : cin, cout);
    }
    for (int i = 0; i < c.inter_layers; ++i) {
        const int cin = i == 0 ? C << (E - 1) : C << E, cout = C << E;
        for (int k = 0; k < nb; ++k)
            rmvpe_block_names(e, "unet.intermediate.layers." + std::to_string(i) + ".conv." + std::to_string(k), k ? cout : cin, cout);
    }
    for (int i = 0; i < E; ++i) {
        const int cin = C << (E - i), cout = cin / 2;
        const std::string p = "unet.decoder.layers." + std::to_string(i);
        e.push_back({p + ".conv1.0.weight", {cin, cout, 3, 3}});
        for (auto n : bn) e.push_back({p + ".conv1.1." + n, {cout}});
        for (int k = 0; k < nb; ++k) rmvpe_block_names(e, p + ".conv2." + std::to_string(k), k ? cout : 2 * cout, cout);
    }
    e.push_back({"cnn.weight", {3, C, 3, 3}});
    e.push_back({"cnn.bias", {3}});
    if (c.n_gru) {
        for (std::string sfx : {"", "_reverse"}) {
            e.push_back({"fc.0.gru.weight_ih_l0" + sfx, {768, 3 * RM_MELS}});
            e.push_back({"fc.0.gru.weight_hh_l0" + sfx, {768, 256}});
            e.push_back({"fc.0.gru.bias_ih_l0" + sfx, {768}});
            e.push_back({"fc.0.gru.bias_hh_l0" + sfx, {768}});
        }
        e.push_back({"fc.1.weight", {RM_CLASSES, 512}});
        e.push_back({"fc.1.bias", {RM_CLASSES}});
    } else {
        e.push_back({"fc.0.weight", {RM_CLASSES, 3 * RM_MELS}});
        e.push_back({"fc.0.bias", {RM_CLASSES}});
    }
    return e;
}

}  // namespace

int dsd::rmvpe_load_weight(dsd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim,
                      int32_t on_device) {
    if (!name) return fail(h, DSD_EINVAL, "dsd_load_weight: bad argument");
    const std::string n(name);
    // strict=False in the reference's RMVPE: TimbreFilter is never called in forward; BatchNorm's step counter carries no value
    if (n.rfind("unet.tf.", 0) == 0 || ends_with(n, ".num_batches_tracked")) return DSD_OK;
    if (!data || !shape || ndim < 1 || ndim > 4) return fail(h, DSD_EINVAL, "dsd_load_weight: bad argument");
    RmvpeState& r = *h->pe;
    const int rc = store_weight(h, &r.expected, name, data, shape, ndim, on_device);
    if (rc == DSD_OK) h->finalized = false;
    return rc;
}

namespace {

// a 3x3 conv [cout][cin][3][3] (transposed: [cin][cout][3][3]) with the BN scale folded in -> [tap][cin][cout_pad]
RmConvW rmvpe_pack_conv(std::vector<float>& blob, const std::vector<float>& w, int cin, int cout, bool transposed,
                        const std::vector<double>& sc, const std::vector<double>& sh) {
    RmConvW c;
    c.cin = cin;
    c.cout = cout;
    c.cout_pad = (cout + 7) / 8 * 8;
    c.w = blob.size();
    blob.resize(blob.size() + (size_t)9 * cin * c.cout_pad, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                const float v = transposed ? w[((size_t)ci * cout + co) * 9 + tap] : w[((size_t)co * cin + ci) * 9 + tap];
                blob[c.w + ((size_t)tap * cin + ci) * c.cout_pad + co] = (float)((double)v * sc[co]);
            }
    c.shift = blob.size();
    blob.resize(blob.size() + c.cout_pad, 0.f);
    for (int co = 0; co < cout; ++co) blob[c.shift + co] = (float)sh[co];
    return c;
}

RmBlockW rmvpe_pack_block(const dsd_handle* h, std::vector<float>& blob, const std::string& p, int cin, int cout) {
    std::vector<double> sc, sh;
    RmBlockW b;
    bn_scale_shift(h, p + ".conv.1", cout, sc, sh);
    b.c1 = rmvpe_pack_conv(blob, h->raw.at(p + ".conv.0.weight").data, cin, cout, false, sc, sh);
    bn_scale_shift(h, p + ".conv.4", cout, sc, sh);
    b.c2 = rmvpe_pack_conv(blob, h->raw.at(p + ".conv.3.weight").data, cout, cout, false, sc, sh);
    if (cin != cout) {
        const auto &ws = h->raw.at(p + ".shortcut.weight").data, &bs = h->raw.at(p + ".shortcut.bias").data;
        const int cp = b.c2.cout_pad;
        b.c2.sc = true;
        b.c2.ws = blob.size();
        blob.resize(blob.size() + (size_t)cin * cp, 0.f);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) blob[b.c2.ws + (size_t)ci * cp + co] = ws[(size_t)co * cin + ci];
        b.c2.bs = blob.size();
        blob.resize(blob.size() + cp, 0.f);
        for (int co = 0; co < cout; ++co) blob[b.c2.bs + co] = bs[co];
    }
    return b;
}

// W [N][K] with K indexed c * 128 + f (transpose(1, 2).flatten(-2) of the head's [3][T][128]) -> rows f * 3 + c, the
// head's [frame][bin][channel] order; columns n0 .. n0 + N of a [K][ld] block
void rmvpe_pack_fc(std::vector<float>& blob, size_t at, const std::vector<float>& w, int N, int K, int ld, int n0, bool head_order) {
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            const int kk = head_order ? (k % RM_MELS) * 3 + k / RM_MELS : k;
            blob[at + (size_t)kk * ld + n0 + n] = w[(size_t)n * K + k];
        }
}

}  // namespace

int dsd::rmvpe_finalize(dsd_handle* h) {
    RmvpeState& r = *h->pe;
    const dsd_rmvpe_config& c = r.cfg;
    int rc = check_missing(h, r.expected);
    if (rc) return rc;
    const int E = c.en_de_layers, C = c.en_out_channels, nb = c.n_blocks;
    std::vector<float> blob;
    std::vector<double> sc, sh;
    bn_scale_shift(h, "unet.encoder.bn", 1, sc, sh);
    r.bn0_scale = (float)sc[0];
    r.bn0_shift = (float)sh[0];
    r.enc.assign(E, {});
    for (int l = 0; l < E; ++l) {
        const int cin = l == 0 ? 1 : C << (l - 1), cout = C << l;
        for (int k = 0; k < nb; ++k)
            r.enc[l].push_back(rmvpe_pack_block(h, blob, "unet.encoder.layers." + std::to_string(l) + ".conv." + std::to_string(k),
                                                k ? cout : cin, cout));
    }
    r.inter.assign(c.inter_layers, {});
    for (int i = 0; i < c.inter_layers; ++i) {
        const int cin = i == 0 ? C << (E - 1) : C << E, cout = C << E;
        for (int k = 0; k < nb; ++k)
            r.inter[i].push_back(rmvpe_pack_block(h, blob, "unet.intermediate.layers." + std::to_string(i) + ".conv." +
                                                  std::to_string(k), k ? cout : cin, cout));
    }
    r.dec.assign(E, {});
    r.up.clear();
    for (int i = 0; i < E; ++i) {
        const int cin = C << (E - i), cout = cin / 2;
        const std::string p = "unet.decoder.layers." + std::to_string(i);
        bn_scale_shift(h, p + ".conv1.1", cout, sc, sh);
        r.up.push_back(rmvpe_pack_conv(blob, h->raw.at(p + ".conv1.0.weight").data, cin, cout, true, sc, sh));
        for (int k = 0; k < nb; ++k)
            r.dec[i].push_back(rmvpe_pack_block(h, blob, p + ".conv2." + std::to_string(k), k ? cout : 2 * cout, cout));
    }
    {
        std::vector<double> one(3, 1.0), bias(3);
        for (int k = 0; k < 3; ++k) bias[k] = h->raw.at("cnn.bias").data[k];
        r.head = rmvpe_pack_conv(blob, h->raw.at("cnn.weight").data, C, 3, false, one, bias);
    }
    const int KH = 3 * RM_MELS;
    if (c.n_gru) {
        r.wih = blob.size();
        blob.resize(blob.size() + (size_t)KH * 1536, 0.f);
        r.bih = blob.size();
        blob.resize(blob.size() + 1536, 0.f);
        r.whh = blob.size();
        blob.resize(blob.size() + (size_t)2 * 256 * 768, 0.f);
        r.bhh = blob.size();
        blob.resize(blob.size() + 2 * 768, 0.f);
        for (int d = 0; d < 2; ++d) {
            const std::string sfx = d ? "_reverse" : "";
            rmvpe_pack_fc(blob, r.wih, h->raw.at("fc.0.gru.weight_ih_l0" + sfx).data, 768, KH, 1536, 768 * d, true);
            const auto& bi = h->raw.at("fc.0.gru.bias_ih_l0" + sfx).data;
            const auto& bh = h->raw.at("fc.0.gru.bias_hh_l0" + sfx).data;
            const auto& wh = h->raw.at("fc.0.gru.weight_hh_l0" + sfx).data;
            for (int n = 0; n < 768; ++n) {
                blob[r.bih + 768 * d + n] = bi[n];
                blob[r.bhh + 768 * d + n] = bh[n];
                for (int k = 0; k < 256; ++k) blob[r.whh + ((size_t)d * 256 + k) * 768 + n] = wh[(size_t)n * 256 + k];
            }
        }
        r.fcw = blob.size();
        blob.resize(blob.size() + (size_t)512 * RM_CLASSES, 0.f);
        rmvpe_pack_fc(blob, r.fcw, h->raw.at("fc.1.weight").data, RM_CLASSES, 512, RM_CLASSES, 0, false);
        r.fcb = blob.size();
        blob.insert(blob.end(), h->raw.at("fc.1.bias").data.begin(), h->raw.at("fc.1.bias").data.end());
    } else {
        r.fcw = blob.size();
        blob.resize(blob.size() + (size_t)KH * RM_CLASSES, 0.f);
        rmvpe_pack_fc(blob, r.fcw, h->raw.at("fc.0.weight").data, RM_CLASSES, KH, RM_CLASSES, 0, true);
        r.fcb = blob.size();
        blob.insert(blob.end(), h->raw.at("fc.0.bias").data.begin(), h->raw.at("fc.0.bias").data.end());
    }
    HIP_OK(h, hipSetDevice(h->cfg.device));
    if ((rc = upload_blob(h, r.blob, blob, 0))) return rc;
    h->finalized = true;
    return DSD_OK;
}

void dsd::rmvpe_free(RmvpeState* r) {
    if (r) mel_state_free(r->mel);
    delete r;
}

namespace {

#define RM_LAUNCH(expr, what)                                                                            \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(h, DSD_EHIP, "%s launch failed: %s", what, hipGetErrorString(e_)); \
    } while (0)

// E2E0.forward over each item's Tp_b = 32 ceil(T_b / 32) frames of the log-mel (element (b, m, t) at mel + b sb + m sm + t st),
// then decode.  f0 / hidden_out may be NULL.  `extra` floats at the end of the workspace are left to the caller (front end).
int rmvpe_run(dsd_handle* h, const float* mel, int64_t sb, int64_t sm, int64_t st_, int B, const std::vector<int>& T,
              float thred, float* f0, int64_t f_sb, float* hidden_out, int64_t o_sb, int64_t o_st, hipStream_t st,
              const char* who) {
    RmvpeState& r = *h->pe;
    const dsd_rmvpe_config& c = r.cfg;
    const int E = c.en_de_layers, C = c.en_out_channels;
    std::vector<int> Tp(B);
    int Tpmax = 0, Tmax = 0;
    for (int b = 0; b < B; ++b) {
        Tp[b] = (T[b] + 31) / 32 * 32;
        Tpmax = std::max(Tpmax, Tp[b]);
        Tmax = std::max(Tmax, T[b]);
    }
    // workspace: the prepared input, one skip tensor per encoder level, three rotating tensors, the sigmoid output
    auto level_size = [&](int l, int ch) { return (size_t)B * (size_t)(Tpmax >> l) * (size_t)(RM_MELS >> l) * (size_t)ch; };
    size_t S = (size_t)B * Tpmax * 1536;
    for (int l = 0; l <= E; ++l) S = std::max(S, level_size(l, C << l));
    if (S * 4 >= ((size_t)1 << 31)) return fail(h, DSD_EINVAL, "%s: batch too large for one call (%zu floats per tensor)", who, S);
    std::vector<size_t> skip_off(E);
    size_t n = level_size(0, 1);
    for (int l = 0; l < E; ++l) {
        skip_off[l] = n;
        n += level_size(l, C << l);
    }
    const size_t scr_off = n;
    n += 3 * S;
    const size_t hid_off = n;
    n += (size_t)B * Tpmax * RM_CLASSES;
    int rc = r.ws.reserve(h, n, who);
    if (rc) return rc;
    float* ws = r.ws.p;
    // per-item counts and work lists: conv (quads) and tconv (positions) per level, linear (frames)
    std::vector<int>& iw = r.iw_host;       // kept on the handle: the upload is asynchronous
    iw.assign(2 * B, 0);
    for (int b = 0; b < B; ++b) {
        iw[b] = T[b];
        iw[B + b] = Tp[b];
    }
    std::vector<size_t> conv_wl(E + 1), conv_n(E + 1), tc_wl(E + 1), tc_n(E + 1);
    for (int l = 0; l <= E; ++l) {
        const int F = RM_MELS >> l;
        conv_wl[l] = iw.size();
        for (int b = 0; b < B; ++b) {
            const int Tl = Tp[b] >> l, nq = ((Tl + 1) / 2) * (F / 2);
            for (int q0 = 0; q0 < nq; q0 += 256) iw.insert(iw.end(), {b, q0, Tl});
        }
        conv_n[l] = (iw.size() - conv_wl[l]) / 3;
        tc_wl[l] = iw.size();
        for (int b = 0; b < B; ++b) {
            const int Tl = Tp[b] >> l, np_ = Tl * F;
            for (int q0 = 0; q0 < np_; q0 += 256) iw.insert(iw.end(), {b, q0, Tl});
        }
        tc_n[l] = (iw.size() - tc_wl[l]) / 3;
    }
    const size_t lin_wl = iw.size();
    for (int b = 0; b < B; ++b)
        for (int t0 = 0; t0 < Tp[b]; t0 += 256) iw.insert(iw.end(), {b, t0, Tp[b]});
    const size_t lin_n = (iw.size() - lin_wl) / 3;
    if ((rc = r.iws.reserve(h, iw.size(), who))) return rc;
    HIP_OK(h, hipMemcpyAsync(r.iws.p, iw.data(), iw.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const int *dT = r.iws.p, *dTp = r.iws.p + B;
    const float* wb = r.blob.p;

    RmPrepP pp;
    pp.mel = mel;
    pp.sb = (long)sb;
    pp.sm = (long)sm;
    pp.st = (long)st_;
    pp.T = dT;
    pp.Tp = dTp;
    pp.scale = r.bn0_scale;
    pp.shift = r.bn0_shift;
    pp.x = ws;
    pp.Tal = Tpmax;
    RM_LAUNCH(launch_rm_prep(pp, B, Tpmax, st), "rmvpe prep");

    float* scr[3] = {ws + scr_off, ws + scr_off + S, ws + scr_off + 2 * S};
    auto other = [&](const float* a, const float* b, const float* c = nullptr) -> float* {     // a scratch tensor not a, b, c
        for (float* p : scr)
            if (p != a && p != b && p != c) return p;
        return nullptr;
    };
    auto conv = [&](const RmConvW& cw, int l, const float* x0, int c0, const float* x1, int c1, const float* r0, int rc0,
                    const float* r1, int rc1, int res_mode, bool relu, float* y, float* pool) -> int {
        RmConvP p;
        p.x0 = x0;
        p.x1 = x1;
        p.c0 = c0;
        p.c1 = c1;
        p.r0 = r0;
        p.r1 = r1;
        p.rc0 = rc0;
        p.rc1 = rc1;
        p.res_mode = res_mode;
        p.w = wb + cw.w;
        p.shift = wb + cw.shift;
        p.ws = cw.sc ? wb + cw.ws : nullptr;
        p.bs = cw.sc ? wb + cw.bs : nullptr;
        p.cout = cw.cout;
        p.cout_pad = cw.cout_pad;
        p.relu = relu ? 1 : 0;
        p.F = RM_MELS >> l;
        p.Tal = Tpmax >> l;
        p.y = y;
        p.pool = pool;
        p.work = r.iws.p + conv_wl[l];
        RM_LAUNCH(launch_rm_conv3(p, (int)conv_n[l], st), "rmvpe conv");
        return DSD_OK;
    };
    // ConvBlockRes on x (x0 | x1) at level l -> y; the last block of an encoder layer also writes the pooled tensor
    auto block = [&](const RmBlockW& bw, int l, const float* x0, int c0, const float* x1, int c1, float* y, float* pool) -> int {
        float* h1 = other(x0, y, pool);      // x1 is a skip tensor, never scratch
        int rc2 = conv(bw.c1, l, x0, c0, x1, c1, nullptr, 0, nullptr, 0, 0, true, h1, nullptr);
        if (rc2) return rc2;
        return conv(bw.c2, l, h1, bw.c2.cout, nullptr, 0, x0, c0, x1, c1, bw.c2.sc ? 2 : 1, true, y, pool);
    };
    const float* cur = ws;
    int cc = 1;
    for (int l = 0; l < E; ++l) {
        const int nbk = (int)r.enc[l].size();
        for (int k = 0; k < nbk; ++k) {
            const bool last = k == nbk - 1;
            float* y = last ? ws + skip_off[l] : other(cur, nullptr);
            float* pool = last ? other(cur, nullptr) : nullptr;
            if ((rc = block(r.enc[l][k], l, cur, cc, nullptr, 0, y, pool))) return rc;
            cur = last ? pool : y;
            cc = C << l;
        }
    }
    for (auto& layer : r.inter)
        for (auto& bw : layer) {
            float* y = other(cur, nullptr);
            if ((rc = block(bw, E, cur, cc, nullptr, 0, y, nullptr))) return rc;
            cur = y;
            cc = bw.c2.cout;
        }
    for (int i = 0; i < E; ++i) {
        const int lin = E - i, lo = lin - 1;
        const RmConvW& uw = r.up[i];
        float* u = other(cur, nullptr);
        RmConvP p;
        memset(&p, 0, sizeof(p));
        p.x0 = cur;
        p.c0 = cc;
        p.w = wb + uw.w;
        p.shift = wb + uw.shift;
        p.cout = uw.cout;
        p.cout_pad = uw.cout_pad;
        p.relu = 1;
        p.F = RM_MELS >> lin;
        p.Tal = Tpmax >> lin;
        p.y = u;
        p.work = r.iws.p + tc_wl[lin];
        RM_LAUNCH(launch_rm_tconv(p, (int)tc_n[lin], st), "rmvpe tconv");
        const float* x0 = u;
        const float* x1 = ws + skip_off[lo];
        int c0 = uw.cout, c1 = uw.cout;
        for (auto& bw : r.dec[i]) {
            float* y = other(x0, nullptr);
            if ((rc = block(bw, lo, x0, c0, x1, c1, y, nullptr))) return rc;
            x0 = y;
            x1 = nullptr;
            c0 = bw.c2.cout;
            c1 = 0;
        }
        cur = x0;
        cc = c0;
    }
    float* hd = other(cur, nullptr);
    if ((rc = conv(r.head, 0, cur, cc, nullptr, 0, nullptr, 0, nullptr, 0, 0, false, hd, nullptr))) return rc;
    float* hid = ws + hid_off;
    RmLinearP lp;
    lp.Tal = Tpmax;
    lp.work = r.iws.p + lin_wl;
    if (c.n_gru) {
        float* gi = other(hd, nullptr);
        lp.x = hd;
        lp.w = wb + r.wih;
        lp.bias = wb + r.bih;
        lp.K = 3 * RM_MELS;
        lp.N = 1536;
        lp.act = 0;
        lp.y = gi;
        RM_LAUNCH(launch_rm_linear(lp, (int)lin_n, st), "rmvpe gru input");
        float* gy = other(hd, gi);
        RmGruP gp;
        gp.gi = gi;
        gp.whh = wb + r.whh;
        gp.bhh = wb + r.bhh;
        gp.Tp = dTp;
        gp.Tal = Tpmax;
        gp.y = gy;
        RM_LAUNCH(launch_rm_gru(gp, B, st), "rmvpe gru");
        lp.x = gy;
        lp.K = 512;
    } else {
        lp.x = hd;
        lp.K = 3 * RM_MELS;
    }
    lp.w = wb + r.fcw;
    lp.bias = wb + r.fcb;
    lp.N = RM_CLASSES;
    lp.act = 1;
    lp.y = hid;
    RM_LAUNCH(launch_rm_linear(lp, (int)lin_n, st), "rmvpe fc");
    RmDecodeP dp;
    dp.hidden = hid;
    dp.h_sb = (long)Tpmax * RM_CLASSES;
    dp.h_st = RM_CLASSES;
    dp.T = dT;
    dp.B = B;
    dp.Tmax = Tmax;
    dp.thred = thred;
    dp.f0 = f0;
    dp.f_sb = (long)f_sb;
    dp.out_hidden = hidden_out;
    dp.o_sb = (long)o_sb;
    dp.o_st = (long)o_st;
    dp.center = nullptr;
    dp.c_sb = 0;
    RM_LAUNCH(launch_rm_decode(dp, st), "rmvpe decode");
    return DSD_OK;
}

// torchaudio.functional._get_sinc_resample_kernel(sr, 16000, gcd, lowpass_filter_width=128, rolloff=0.99,
// "sinc_interp_hann") restated: float64 except the phase term, which torch computes as an int64 arange / new_freq (a
// float32 tensor) before adding the float64 tap index; stored as float32.
const RmvpeState::Resampler* rmvpe_resampler(dsd_handle* h, int sr) {
    RmvpeState& r = *h->pe;
    for (auto& x : r.rs)
        if (x.sr == sr) return &x;
    const int g = std::gcd(sr, 16000), orig = sr / g, nw = 16000 / g;
    const double lpw = 128.0, base = std::min(orig, nw) * 0.99;
    const int width = (int)ceil(lpw * orig / base), K = 2 * width + orig;
    std::vector<float> kern((size_t)nw * K);
    for (int p = 0; p < nw; ++p)
        for (int k = 0; k < K; ++k) {
            const double idx = (double)(k - width) / orig;
            double t = ((double)((float)(-p) / (float)nw) + idx) * base;
            t = std::min(lpw, std::max(-lpw, t));
            const double cw = cos(t * M_PI / lpw / 2);
            const double window = cw * cw;
            t *= M_PI;
            const double v = t == 0.0 ? 1.0 : sin(t) / t;
            kern[(size_t)p * K + k] = (float)(v * (window * (base / orig)));
        }
    RmvpeState::Resampler x;
    x.sr = sr;
    x.orig = orig;
    x.nw = nw;
    x.width = width;
    x.K = K;
    if (x.dev.reserve(h, kern.size(), "rmvpe_resampler") ||
        hipMemcpy(x.dev.p, kern.data(), kern.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    r.rs.push_back(std::move(x));
    return &r.rs.back();
}

// to_local_average_f0 around the argmax (centers NULL) or around centers[b * c_stride_b + t]
int rmvpe_decode_frames(dsd_handle* h, const char* who, const float* hidden, const int* centers, int B, int T, int64_t h_stride_b,
                        int64_t h_stride_t, int64_t c_stride_b, float thred, float* f0_out, int64_t f0_stride_b, void* stream) {
    RmvpeState& r = *h->pe;
    std::vector<int>& iw = r.iw_host;
    iw.assign(B, T);
    int rc = r.iws.reserve(h, iw.size(), who);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(h, hipMemcpyAsync(r.iws.p, iw.data(), iw.size() * sizeof(int), hipMemcpyHostToDevice, st));
    RmDecodeP dp;
    dp.hidden = hidden;
    dp.h_sb = (long)h_stride_b;
    dp.h_st = (long)h_stride_t;
    dp.T = r.iws.p;
    dp.B = B;
    dp.Tmax = T;
    dp.thred = thred;
    dp.f0 = f0_out;
    dp.f_sb = (long)f0_stride_b;
    dp.out_hidden = nullptr;
    dp.o_sb = dp.o_st = 0;
    dp.center = centers;
    dp.c_sb = (long)c_stride_b;
    RM_LAUNCH(launch_rm_decode(dp, st), "rmvpe decode");
    return DSD_OK;
}

// The Viterbi decode keeps 360 doubles of log_prob and 360 two-byte back-pointers per frame: 3,600 bytes
constexpr int RM_VT_MAX_T = 131072;
constexpr int64_t RM_VT_MAX_FRAMES = 1 << 20;
// librosa.util.tiny of the float32 probabilities (utils.py:35 hands librosa a float32 array)
constexpr double RM_VT_EPS = (double)FLT_MIN;

// log(transition + eps) of utils.py:29-31 in float64, the band of column j as tab[d + 29][j] = log_trans[j + d][j]: row k is
// divided by its own sum, which is smaller for the 29 rows at either end, so the matrix is not Toeplitz
int rmvpe_viterbi_table(dsd_handle* h, const char* who) {
    RmvpeState& r = *h->pe;
    if (r.vt_tab.p) return DSD_OK;
    std::vector<double> tab((size_t)RM_VT_W * RM_CLASSES, 0.0);
    for (int k = 0; k < RM_CLASSES; ++k) {
        long sum = 0;
        for (int j = 0; j < RM_CLASSES; ++j) sum += std::max(30 - std::abs(k - j), 0);
        for (int j = std::max(k - RM_VT_BAND, 0); j <= std::min(k + RM_VT_BAND, RM_CLASSES - 1); ++j)
            tab[(size_t)(k - j + RM_VT_BAND) * RM_CLASSES + j] = log((double)(30 - std::abs(k - j)) / (double)sum + RM_VT_EPS);
    }
    int rc = r.vt_tab.reserve(h, tab.size(), who);
    if (rc) return rc;
    if (hipMemcpy(r.vt_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        r.vt_tab = DevBuf<double>();
        return fail(h, DSD_EHIP, "%s: the transition table could not be placed on the device", who);
    }
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_rmvpe_create(const dsd_rmvpe_config* cfg, dsd_handle** out) {
    int rc = create_check(cfg, out, "dsd_rmvpe_create", [](const dsd_rmvpe_config* c) {
        if (c->n_blocks < 1 || (c->n_gru != 0 && c->n_gru != 1) || c->en_de_layers < 1 || c->en_de_layers > 5 ||
            c->inter_layers < 1 || c->en_out_channels < 8 || c->en_out_channels % 8 != 0 || c->en_out_channels > 64)
            return fail(nullptr, DSD_EINVAL, "dsd_rmvpe_create: need n_blocks >= 1, n_gru in {0, 1}, 1 <= en_de_layers <= 5, "
                        "inter_layers >= 1 and en_out_channels a multiple of 8 in [8, 64]");
        return DSD_OK;
    });
    if (rc) return rc;
    dsd_handle* h = new_handle(DSD_PE_RMVPE, cfg->device);
    h->cfg.in_dims = RM_MELS;
    h->cfg.n_feats = 1;
    h->pe = new RmvpeState();
    h->pe->cfg = *cfg;
    h->pe->expected = rmvpe_expected(*cfg);
    const dsd_mel_config mc = rmvpe_mel_config(cfg->device);
    std::vector<float> w;
    mel_filterbank_host(mc, w, true);
    h->pe->mel = new MelState();
    rc = mel_state_build(*h->pe->mel, &mc, w, "dsd_rmvpe_create");
    if (rc) {
        dsd_destroy(h);
        return rc;
    }
    *out = h;
    return DSD_OK;
}

int64_t dsd_rmvpe_num_frames(int64_t n_samples, int32_t sample_rate) {
    if (sample_rate < 1 || n_samples < 1) return fail(nullptr, DSD_EINVAL, "dsd_rmvpe_num_frames: need n_samples, sample_rate >= 1");
    const int64_t L16 = rmvpe_resampled_length(n_samples, sample_rate);
    const int64_t T = mel_frames(rmvpe_geometry(), L16);
    if (T < 1)
        return fail(nullptr, DSD_EINVAL, "dsd_rmvpe_num_frames: %lld samples at 16 kHz are too short (torch.stft's reflect pad "
                    "of 512 raises)", (long long)L16);
    return T;
}

int dsd_rmvpe_filterbank(float* out) {
    if (!out) return fail(nullptr, DSD_EINVAL, "dsd_rmvpe_filterbank: null output");
    std::vector<float> w;
    mel_filterbank_host(rmvpe_mel_config(0), w, true);
    memcpy(out, w.data(), w.size() * sizeof(float));
    return DSD_OK;
}

int dsd_rmvpe_mel_to_hidden(dsd_handle* h, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_m,
                         int64_t stride_t, const int64_t* lengths, float* hidden_out, int64_t h_stride_b,
                         int64_t h_stride_t, void* stream) {
    if (!h || !mel || !hidden_out) return fail(h, DSD_EINVAL, "dsd_rmvpe_mel_to_hidden: null argument");
    int rc = enter(h, "dsd_rmvpe_mel_to_hidden", K_PE, ENTER_WEIGHTS | ENTER_LAUNCH);
    if (rc) return rc;
    if (B < 1 || T < 1 || T > (1 << 24)) return fail(h, DSD_EINVAL, "dsd_rmvpe_mel_to_hidden: need B >= 1 and 1 <= T <= 2^24");
    std::vector<int> Tb(B);
    for (int b = 0; b < B; ++b) {
        const int64_t v = lengths ? lengths[b] : T;
        if (v < 1 || v > T) return fail(h, DSD_EINVAL, "dsd_rmvpe_mel_to_hidden: lengths[%d] = %lld outside [1, %d]", b, (long long)v, T);
        Tb[b] = (int)v;
    }
    return rmvpe_run(h, mel, stride_b, stride_m, stride_t, B, Tb, 0.f, nullptr, 0, hidden_out, h_stride_b, h_stride_t,
                     (hipStream_t)stream, "dsd_rmvpe_mel_to_hidden");
}

int dsd_rmvpe_decode(dsd_handle* h, const float* hidden, int32_t B, int32_t T, int64_t h_stride_b, int64_t h_stride_t,
                     float thred, float* f0_out, int64_t f0_stride_b, void* stream) {
    if (!h || !hidden || !f0_out) return fail(h, DSD_EINVAL, "dsd_rmvpe_decode: null argument");
    if (int rc = enter(h, "dsd_rmvpe_decode", K_PE, ENTER_LAUNCH)) return rc;       // no weights: the hidden is the caller's
    if (B < 1 || T < 1 || T > (1 << 24)) return fail(h, DSD_EINVAL, "dsd_rmvpe_decode: need B >= 1 and 1 <= T <= 2^24");
    return rmvpe_decode_frames(h, "dsd_rmvpe_decode", hidden, nullptr, B, T, h_stride_b, h_stride_t, 0, thred, f0_out, f0_stride_b,
                               stream);
}

int dsd_rmvpe_decode_at(dsd_handle* h, const float* hidden, const int32_t* centers, int32_t B, int32_t T, int64_t h_stride_b,
                        int64_t h_stride_t, int64_t c_stride_b, float thred, float* f0_out, int64_t f0_stride_b, void* stream) {
    const char* who = "dsd_rmvpe_decode_at";
    if (!h || !hidden || !centers || !f0_out) return fail(h, DSD_EINVAL, "%s: null argument", who);
    if (int rc = enter(h, who, K_PE, ENTER_LAUNCH)) return rc;
    if (B < 1 || T < 1 || T > RM_VT_MAX_T) return fail(h, DSD_EINVAL, "%s: need B >= 1 and 1 <= T <= %d frames", who, RM_VT_MAX_T);
    return rmvpe_decode_frames(h, who, hidden, centers, B, T, h_stride_b, h_stride_t, c_stride_b, thred, f0_out, f0_stride_b, stream);
}

int dsd_rmvpe_decode_viterbi(dsd_handle* h, const float* hidden, int32_t B, int32_t T, int64_t h_stride_b, int64_t h_stride_t,
                             const int64_t* lengths, float thred, float* f0_out, int64_t f0_stride_b, int32_t* path_out,
                             int64_t path_stride_b, void* stream) {
    const char* who = "dsd_rmvpe_decode_viterbi";
    if (!h || !hidden || !f0_out) return fail(h, DSD_EINVAL, "%s: null argument", who);
    int rc = enter(h, who, K_PE, ENTER_LAUNCH);
    if (rc) return rc;
    if (B < 1 || T < 1 || T > RM_VT_MAX_T || (int64_t)B * T > RM_VT_MAX_FRAMES)
        return fail(h, DSD_EINVAL, "%s: need B >= 1, 1 <= T <= %d frames and B * T <= %lld frames (the back-pointer and log_prob "
                    "workspaces take 3600 bytes per frame)", who, RM_VT_MAX_T, (long long)RM_VT_MAX_FRAMES);
    RmvpeState& r = *h->pe;
    std::vector<int>& iw = r.vt_iw_host;
    iw.resize(B);
    for (int b = 0; b < B; ++b) {
        const int64_t v = lengths ? lengths[b] : T;
        if (v < 1 || v > T) return fail(h, DSD_EINVAL, "%s: lengths[%d] = %lld outside [1, %d]", who, b, (long long)v, T);
        iw[b] = (int)v;
    }
    const size_t frames = (size_t)B * T;
    if ((rc = rmvpe_viterbi_table(h, who)) || (rc = r.vt_lp.reserve(h, frames * RM_CLASSES, who)) ||
        (rc = r.vt_ptr.reserve(h, frames * RM_CLASSES, who)) || (rc = r.vt_iw.reserve(h, B + frames, who)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(h, hipMemcpyAsync(r.vt_iw.p, iw.data(), iw.size() * sizeof(int), hipMemcpyHostToDevice, st));
    RmViterbiP vp;
    vp.hidden = hidden;
    vp.h_sb = (long)h_stride_b;
    vp.h_st = (long)h_stride_t;
    vp.T = r.vt_iw.p;
    vp.B = B;
    vp.Tmax = T;
    vp.tab = r.vt_tab.p;
    vp.eps = RM_VT_EPS;
    vp.log_eps = log(RM_VT_EPS);
    vp.log_p_init = log(1.0 / RM_CLASSES + RM_VT_EPS);
    vp.lp = r.vt_lp.p;
    vp.ptr = r.vt_ptr.p;
    vp.center = r.vt_iw.p + B;
    vp.path_out = path_out;
    vp.p_sb = (long)path_stride_b;
    RM_LAUNCH(launch_rm_viterbi(vp, st), "rmvpe viterbi");
    RmDecodeP dp;
    dp.hidden = hidden;
    dp.h_sb = (long)h_stride_b;
    dp.h_st = (long)h_stride_t;
    dp.T = r.vt_iw.p;
    dp.B = B;
    dp.Tmax = T;
    dp.thred = thred;
    dp.f0 = f0_out;
    dp.f_sb = (long)f0_stride_b;
    dp.out_hidden = nullptr;
    dp.o_sb = dp.o_st = 0;
    dp.center = vp.center;
    dp.c_sb = T;
    RM_LAUNCH(launch_rm_decode(dp, st), "rmvpe decode");
    return DSD_OK;
}

int dsd_rmvpe_infer(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                    const int64_t* lengths, int32_t sample_rate, float thred, float* f0_out, int64_t f0_stride_b,
                    float* hidden_out, int64_t h_stride_b, int64_t h_stride_t, void* stream) {
    const char* who = "dsd_rmvpe_infer";
    if (!h || !wav || !f0_out) return fail(h, DSD_EINVAL, "%s: null argument", who);
    int rc = enter(h, who, K_PE, ENTER_WEIGHTS | ENTER_LAUNCH);
    if (rc) return rc;
    RmvpeState& r = *h->pe;
    if (B < 1 || n_samples < 1 || sample_rate < 1) return fail(h, DSD_EINVAL, "%s: B, n_samples and sample_rate must be positive", who);
    if (n_samples > ((int64_t)1 << 30) || (B > 1 && wav_stride_b < n_samples))
        return fail(h, DSD_EINVAL, "%s: n_samples must be <= 2^30 and wav_stride_b >= n_samples", who);
    std::vector<int64_t> L(B), L16(B);
    std::vector<int> T(B);
    int64_t L16max = 0;
    int Tmax = 0;
    for (int b = 0; b < B; ++b) {
        L[b] = lengths ? lengths[b] : n_samples;
        if (L[b] < 1 || L[b] > n_samples)
            return fail(h, DSD_EINVAL, "%s: lengths[%d] = %lld outside [1, %lld]", who, b, (long long)L[b], (long long)n_samples);
        L16[b] = rmvpe_resampled_length(L[b], sample_rate);
        const int64_t t = mel_frames(rmvpe_geometry(), L16[b]);
        if (t < 1)
            return fail(h, DSD_EINVAL, "%s: item %d has %lld samples at 16 kHz; torch.stft's reflect pad of 512 needs more", who, b,
                        (long long)L16[b]);
        T[b] = (int)t;
        L16max = std::max(L16max, L16[b]);
        Tmax = std::max(Tmax, T[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    // the front end's log-mel and resampled audio live in a block of their own: rmvpe_run reuses the workspace
    const float* w16 = wav;
    int64_t w16_sb = wav_stride_b;
    const size_t mel_n = (size_t)B * RM_MELS * Tmax, wav_n = sample_rate == 16000 ? 0 : (size_t)B * L16max;
    if ((rc = r.fe.reserve(h, mel_n + wav_n, who))) return rc;
    float* front = r.fe.p;
    if (sample_rate != 16000) {
        const RmvpeState::Resampler* rs = rmvpe_resampler(h, sample_rate);
        if (!rs) return fail(h, DSD_ENOMEM, "%s: the resampling kernel for %d Hz could not be placed on the device", who, sample_rate);
        std::vector<int>& lens = r.lens_host;
        lens.resize(2 * B);
        for (int b = 0; b < B; ++b) {
            lens[b] = (int)L[b];
            lens[B + b] = (int)L16[b];
        }
        if ((rc = r.lens.reserve(h, lens.size(), who))) return rc;
        HIP_OK(h, hipMemcpyAsync(r.lens.p, lens.data(), lens.size() * sizeof(int), hipMemcpyHostToDevice, st));
        RmResampleP p;
        p.x = wav;
        p.x_sb = (long)wav_stride_b;
        p.len_in = r.lens.p;
        p.len_out = r.lens.p + B;
        p.kern = rs->dev.p;
        p.K = rs->K;
        p.orig = rs->orig;
        p.nw = rs->nw;
        p.width = rs->width;
        p.y = front + mel_n;
        p.y_sb = (long)L16max;
        RM_LAUNCH(launch_rm_resample(p, B, (L16max + rs->nw - 1) / rs->nw, rs->nw, st), "rmvpe resample");
        w16 = front + mel_n;
        w16_sb = L16max;
    }
    rc = mel_run(h, *r.mel, rmvpe_geometry(), w16, B, L16max, w16_sb, L16.data(), front, (int64_t)RM_MELS * Tmax, Tmax, 1,
                 stream, who);
    if (rc) return rc;
    rc = rmvpe_run(h, front, (int64_t)RM_MELS * Tmax, Tmax, 1, B, T, thred, f0_out, f0_stride_b, hidden_out, h_stride_b,
                   h_stride_t, st, who);
    return rc;
}

}  // extern "C"
