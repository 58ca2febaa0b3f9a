// libdsdenoise, host side of mel analysis: dsd_mel_create, dsd_mel_filterbank, dsd_mel_num_frames, dsd_mel_analyze
// (kernels: mel_kernels.hip).  RMVPE's front end (rmvpe_api.hip) runs the same analysis through mel_run.
#include "api_host.h"

// ------------------------------------------------------------------------------------------------------------------------------
// Mel analysis (dsd_mel_*): STFT.get_mel, modules/nsf_hifigan/nvSTFT.py:50-87
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

int mel_check_config(const dsd_mel_config* c, const char* who) {
    if (!c) return fail(nullptr, DSD_EINVAL, "%s: null config", who);
    if (c->struct_size != (int32_t)sizeof(dsd_mel_config))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, c->struct_size, sizeof(dsd_mel_config));
    if (c->sampling_rate < 1 || c->n_fft < 2 || c->n_fft > 16384 || c->win_size < 1 || c->win_size > c->n_fft ||
        c->hop_size < 1 || c->num_mels < 1 || c->num_mels > 1024)
        return fail(nullptr, DSD_EINVAL, "%s: need sampling_rate >= 1, 2 <= n_fft <= 16384, 1 <= win_size <= n_fft, hop_size >= 1 "
                    "and 1 <= num_mels <= 1024", who);
    if (!(c->fmin >= 0.0) || !(c->fmax > c->fmin) || !std::isfinite(c->fmax))
        return fail(nullptr, DSD_EINVAL, "%s: need 0 <= fmin < fmax (got %g, %g)", who, c->fmin, c->fmax);
    if (!(c->clip_val > 0.0) || !std::isfinite(c->clip_val)) return fail(nullptr, DSD_EINVAL, "%s: clip_val must be > 0", who);
    return DSD_OK;
}

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults (htk=False, norm="slaney", dtype=float32), restated
// step by step in float64 as librosa computes it: Slaney scale (linear at 200/3 Hz per mel below 1000 Hz = 15 mel,
// logarithmic above with step ln(6.4) / 27), np.linspace of the mel points, np.fft.rfftfreq bin centres, triangles stored
// into the float32 array, then the area normalisation 2 / (f[i+2] - f[i]) multiplied in place (a float32 result).
double slaney_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
double slaney_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}
// htk = true: librosa's HTK scale instead (mel = 2595 log10(1 + f / 700)), the same triangles and Slaney area norm
double htk_hz_to_mel(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
double htk_mel_to_hz(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }

}  // namespace

namespace dsd {

void mel_filterbank_host(const dsd_mel_config& c, std::vector<float>& w, bool htk) {
    const int M = c.num_mels, K = c.n_fft / 2 + 1, n = M + 2;
    double (*to_mel)(double) = htk ? htk_hz_to_mel : slaney_hz_to_mel;
    double (*to_hz)(double) = htk ? htk_mel_to_hz : slaney_mel_to_hz;
    const double lo = to_mel(c.fmin), hi = to_mel(c.fmax), step = (hi - lo) / (double)(n - 1);
    std::vector<double> mel_f(n), fft_f(K);
    for (int i = 0; i < n; ++i) {
        const double m = (double)i * step;      // np.linspace: arange * step + start, the end point set to stop
        mel_f[i] = to_hz(i == n - 1 ? hi : m + lo);
    }
    const double val = 1.0 / ((double)c.n_fft * (1.0 / (double)c.sampling_rate));      // np.fft.rfftfreq(n_fft, 1 / sr)
    for (int k = 0; k < K; ++k) fft_f[k] = (double)k * val;
    w.assign((size_t)M * K, 0.f);
    for (int i = 0; i < M; ++i) {
        const double d0 = mel_f[i + 1] - mel_f[i], d1 = mel_f[i + 2] - mel_f[i + 1], enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < K; ++k) {
            const double lower = -(mel_f[i] - fft_f[k]) / d0, upper = (mel_f[i + 2] - fft_f[k]) / d1;
            const float tri = (float)std::max(0.0, std::min(lower, upper));
            w[(size_t)i * K + k] = (float)((double)tri * enorm);
        }
    }
}

bool mel_geometry(const dsd_mel_config& c, double keyshift, double speed, MelGeom& g) {
    if (!std::isfinite(keyshift) || !std::isfinite(speed) || !(speed > 0.0)) return false;
    const double factor = pow(2.0, keyshift / 12.0);
    const double N = nearbyint(c.n_fft * factor), W = nearbyint(c.win_size * factor), H = nearbyint(c.hop_size * speed);
    if (!(N >= 1 && N <= 32768 && W >= 1 && W <= N && H >= 1 && H <= (1 << 24))) return false;
    g.N = (int)N;
    g.W = (int)W;
    g.H = (int)H;
    g.off = (g.N - g.W) / 2;                               // torch.stft centres a shorter window in the frame
    const int d = g.W - g.H;                               // Python floor division of d and d + 1 by 2
    g.padL = d >= 0 ? d / 2 : -((-d + 1) / 2);
    g.padR = d + 1 >= 0 ? (d + 1) / 2 : -((-(d + 1) + 1) / 2);
    g.rescale = keyshift != 0.0;
    return true;
}
// T of an item of L samples, or -1 where torch raises (reflect pad >= L, padded signal shorter than N')
int64_t mel_frames(const MelGeom& g, int64_t L) {
    if (L < 1 || g.padL >= L || g.padR >= L) return -1;
    const int64_t Lp = L + g.padL + g.padR;
    if (Lp < g.N) return -1;
    return 1 + (Lp - g.N) / g.H;
}

// the packed non-zero runs of the filterbank w [num_mels][n_fft / 2 + 1] on the device
int mel_state_build(MelState& mst, const dsd_mel_config* cfg, const std::vector<float>& w, const char* who) {
    // the non-zero run of every filter (librosa's triangles are contiguous), packed
    const int M = cfg->num_mels, K = cfg->n_fft / 2 + 1;
    std::vector<int> first(M, -1), last(M, -2);
    int k_lo = K, k_hi = -1;
    for (int m = 0; m < M; ++m) {
        for (int k = 0; k < K; ++k)
            if (w[(size_t)m * K + k] != 0.f) {
                if (first[m] < 0) first[m] = k;
                last[m] = k;
            }
        if (first[m] >= 0) {
            k_lo = std::min(k_lo, first[m]);
            k_hi = std::max(k_hi, last[m]);
        }
    }
    if (k_hi < 0) k_lo = 0;
    std::vector<int> range(2 * M), woff(M);
    std::vector<float> fw;
    for (int m = 0; m < M; ++m) {
        woff[m] = (int)fw.size();
        if (first[m] < 0) {
            range[2 * m] = range[2 * m + 1] = 0;
            continue;
        }
        range[2 * m] = first[m] - k_lo;
        range[2 * m + 1] = last[m] + 1 - k_lo;
        for (int k = first[m]; k <= last[m]; ++k) fw.push_back(w[(size_t)m * K + k]);
    }
    fw.push_back(0.f);       // never empty
    MelState* ms = &mst;
    ms->cfg = *cfg;
    ms->k_lo = k_lo;
    ms->k_hi = k_hi;
    ms->range_host = range;
    if (ms->range.reserve(nullptr, range.size(), who) || ms->woff.reserve(nullptr, M, who) || ms->fw.reserve(nullptr, fw.size(), who))
        return DSD_ENOMEM;
    if (hipMemcpy(ms->range.p, range.data(), sizeof(int) * range.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ms->woff.p, woff.data(), sizeof(int) * M, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ms->fw.p, fw.data(), sizeof(float) * fw.size(), hipMemcpyHostToDevice) != hipSuccess) {
        return fail(nullptr, DSD_EHIP, "%s: upload of the filterbank failed", who);
    }
    return DSD_OK;
}

void mel_state_free(MelState* m) { delete m; }

}  // namespace dsd

extern "C" {

int dsd_mel_filterbank(const dsd_mel_config* cfg, float* out) {
    int rc = mel_check_config(cfg, "dsd_mel_filterbank");
    if (rc) return rc;
    if (!out) return fail(nullptr, DSD_EINVAL, "dsd_mel_filterbank: null output");
    std::vector<float> w;
    mel_filterbank_host(*cfg, w);
    memcpy(out, w.data(), w.size() * sizeof(float));
    return DSD_OK;
}

int64_t dsd_mel_num_frames(const dsd_mel_config* cfg, int64_t n_samples, double keyshift, double speed) {
    if (mel_check_config(cfg, "dsd_mel_num_frames")) return DSD_EINVAL;
    MelGeom g;
    if (!mel_geometry(*cfg, keyshift, speed, g)) return fail(nullptr, DSD_EINVAL, "dsd_mel_num_frames: bad keyshift / speed");
    const int64_t T = mel_frames(g, n_samples);
    if (T < 1) return fail(nullptr, DSD_EINVAL, "dsd_mel_num_frames: %lld samples are too short (torch.stft / reflect pad raise)",
                           (long long)n_samples);
    return T;
}

int dsd_mel_create(const dsd_mel_config* cfg, dsd_handle** out) {
    int rc = create_check(cfg, out, "dsd_mel_create", [](const dsd_mel_config* c) { return mel_check_config(c, "dsd_mel_create"); });
    if (rc) return rc;
    dsd_handle* h = new_handle(DSD_MEL_ANALYSIS, cfg->device);
    h->cfg.in_dims = cfg->num_mels;
    h->cfg.n_feats = 1;
    std::vector<float> w;
    mel_filterbank_host(*cfg, w);
    h->mel = new MelState();
    rc = mel_state_build(*h->mel, cfg, w, "dsd_mel_create");
    if (rc) {
        dsd_destroy(h);
        return rc;
    }
    *out = h;
    return DSD_OK;
}

}  // extern "C"

namespace dsd {

// the analysis of dsd_mel_analyze after its entry and argument checks, for one STFT geometry (RMVPE's front end calls it too)
int mel_run(dsd_handle* h, MelState& ms, const MelGeom& g, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
            const int64_t* lengths, float* mel_out, int64_t stride_b, int64_t stride_m, int64_t stride_t, void* stream,
            const char* who) {
    const dsd_mel_config& c = ms.cfg;
    // work list: (item, 64-frame tile) entries over the frames each item has
    std::vector<int>& work = ms.work_host;
    work.clear();
    int64_t G = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = lengths ? lengths[b] : n_samples;
        if (L < 1 || L > n_samples) return fail(h, DSD_EINVAL, "%s: lengths[%d] = %lld outside [1, %lld]", who, b,
                                                (long long)L, (long long)n_samples);
        const int64_t T = mel_frames(g, L);
        if (T < 1)
            return fail(h, DSD_EINVAL, "%s: item %d (%lld samples) is too short for N' = %d, W' = %d, H' = %d "
                        "(torch.stft / reflect pad raise)", who, b, (long long)L, g.N, g.W, g.H);
        for (int64_t t0 = 0; t0 < T; t0 += kDftFrames) {
            const int e[5] = {b, (int)t0, (int)L, (int)T, (int)(G + t0)};
            work.insert(work.end(), e, e + 5);
        }
        G += T;
        if (G > ((int64_t)1 << 30)) return fail(h, DSD_EINVAL, "%s: too many frames in one call", who);
    }
    const int n_entries = (int)(work.size() / 5);
    // bins the filterbank reads that this N' has: nvSTFT.py:76-80 zero-pads the bins past N'/2
    const int k_hi = std::min(ms.k_hi, g.N / 2), nb = std::max(0, k_hi - ms.k_lo + 1);
    const int row_tiles = (2 * nb + kDftRows - 1) / kDftRows, Kpad = (g.W + kDftTaps - 1) / kDftTaps * kDftTaps;
    hipStream_t st = (hipStream_t)stream;
    float* basis = nullptr;
    if (nb > 0) {
        for (size_t i = 0; i < ms.bases.size(); ++i)
            if (ms.bases[i].N == g.N && ms.bases[i].W == g.W) {
                std::rotate(ms.bases.begin() + i, ms.bases.begin() + i + 1, ms.bases.end());      // most recent last
                basis = ms.bases.back().dev.p;
                break;
            }
        if (!basis) {
            if (ms.bases.size() == 4) ms.bases.erase(ms.bases.begin());     // continuous keyshift draws: keep the four most recent sizes
            MelBasis mb;
            mb.N = g.N;
            mb.W = g.W;
            if (int rc = mb.dev.reserve(h, (size_t)row_tiles * kDftRows * Kpad, who)) return rc;
            basis = mb.dev.p;
            ms.bases.push_back(std::move(mb));
            hipError_t e = launch_mel_basis(basis, row_tiles * kDftRows, Kpad, ms.k_lo, nb, g.N, g.W, g.off, st);
            if (e != hipSuccess) return fail(h, DSD_EHIP, "mel basis launch failed: %s", hipGetErrorString(e));
        }
    }
    if (int rc = ms.work.reserve(h, work.size(), who)) return rc;
    HIP_OK(h, hipMemcpyAsync(ms.work.p, work.data(), sizeof(int) * work.size(), hipMemcpyHostToDevice, st));
    const size_t mags_n = std::max<size_t>(1, (size_t)nb * (size_t)G);
    if (int rc = ms.mags.reserve(h, mags_n, who)) return rc;
    if (nb > 0) {
        MelDftP p;
        p.wav = wav;
        p.wav_bstride = (long)wav_stride_b;
        p.work = ms.work.p;
        p.basis = basis;
        p.Kpad = Kpad;
        p.W = g.W;
        p.H = g.H;
        p.off = g.off;
        p.padL = g.padL;
        p.nb = nb;
        p.rescale = g.rescale ? 1 : 0;
        p.win_size = (float)c.win_size;
        p.win_new = (float)g.W;
        p.mags = ms.mags.p;
        p.G = (long)G;
        hipError_t e = launch_mel_dft(p, n_entries, row_tiles, st);
        if (e != hipSuccess) return fail(h, DSD_EHIP, "mel DFT launch failed: %s", hipGetErrorString(e));
    }
    MelProjP q;
    q.work = ms.work.p;
    q.mags = ms.mags.p;
    q.G = (long)G;
    q.nb = nb;
    q.M = c.num_mels;
    q.range = ms.range.p;
    q.woff = ms.woff.p;
    q.fw = ms.fw.p;
    q.clip = (float)c.clip_val;
    q.out = mel_out;
    q.o_sb = (long)stride_b;
    q.o_sm = (long)stride_m;
    q.o_st = (long)stride_t;
    hipError_t e = launch_mel_project(q, n_entries, st);
    if (e != hipSuccess) return fail(h, DSD_EHIP, "mel projection launch failed: %s", hipGetErrorString(e));
    return DSD_OK;
}

}  // namespace dsd

extern "C" int dsd_mel_analyze(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                    const int64_t* lengths, double keyshift, double speed, float* mel_out, int64_t stride_b,
                    int64_t stride_m, int64_t stride_t, void* stream) {
    if (!h || !wav || !mel_out) return fail(h, DSD_EINVAL, "dsd_mel_analyze: null argument");
    if (int rc = enter(h, "dsd_mel_analyze", K_MEL, ENTER_LAUNCH)) return rc;
    MelState& ms = *h->mel;
    const dsd_mel_config& c = ms.cfg;
    if (B < 1 || n_samples < 1) return fail(h, DSD_EINVAL, "dsd_mel_analyze: B and n_samples must be positive (%d, %lld)", B,
                                            (long long)n_samples);
    if (n_samples > ((int64_t)1 << 31) - 1 || (B > 1 && wav_stride_b < n_samples))
        return fail(h, DSD_EINVAL, "dsd_mel_analyze: n_samples must be < 2^31 and wav_stride_b >= n_samples");
    MelGeom g;
    if (!mel_geometry(c, keyshift, speed, g))
        return fail(h, DSD_EINVAL, "dsd_mel_analyze: keyshift %g / speed %g give no valid STFT size", keyshift, speed);
    return mel_run(h, ms, g, wav, B, n_samples, wav_stride_b, lengths, mel_out, stride_b, stride_m, stride_t, stream,
                   "dsd_mel_analyze");
}
