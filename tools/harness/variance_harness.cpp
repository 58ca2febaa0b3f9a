// Stand-alone memory check of the host-only half of dsd_variance_open (diffsinger_amd/csrc/variance_tables.hip), under the
// host compiler's address and undefined-behaviour sanitizers.  Builds tables sections in memory - every tensor its own heap
// allocation of exactly count floats, every name its own exact allocation - for a set of flag combinations, and runs
//   1. the valid section of each combination: DSD_OK, every slot the flags require filled, none the flags exclude;
//   2. each refusal on each combination where it applies: a tensor missing, a tensor the flags exclude, an unknown tensor,
//      every tensor with a dimension one short, one long, transposed or of another rank, a mask value that is not 0 / 1,
//      K outside 1 .. 255, a flag that is not 0 / 1, a wrong struct_size - a negative code and a message naming the tensor
//      or field;
//   3. the inner-config check: valid, and one mismatch per field it compares;
//   4. the taps for every K in 1 .. 255 into a buffer of exactly K floats: finite and summing to 1 for K > 1, NaN for K = 1;
//      the bits of a few K are printed (`taps K hex...`) for the host test to compare with its restatement.
// A read past a tensor (the mask is read to its end), a write past the taps or the index struct is what the sanitizer
// reports.  Host only - never loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/variance_harness.cpp -x c++ diffsinger_amd/csrc/variance_tables.hip -o /tmp/variance_harness
//   /tmp/variance_harness        # prints one line of counts; exit status 0 = clean
//
// The library proper takes dsd::fail from api.hip; this program brings its own.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../diffsinger_amd/csrc/variance_tables.h"

// the layout tests/test_cvariance_host.py pins from the Python side, from the C side
static_assert(sizeof(dsd_variance_config) == 184, "dsd_variance_config is 46 words");
static_assert(offsetof(dsd_variance_config, variances) == 44 && offsetof(dsd_variance_config, glide_embed_scale) == 56 &&
                  offsetof(dsd_variance_config, var_norm_min) == 88 && offsetof(dsd_variance_config, var_no_clamp) == 152 &&
                  offsetof(dsd_variance_config, time_scale_factor) == 180,
              "dsd_variance_config layout");

struct dsd_handle;
static std::string g_error;
namespace dsd {
int fail(dsd_handle*, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}
}  // namespace dsd

static int g_run = 0, g_bad = 0;
static void expect(bool ok, const char* what, const std::string& detail = "") {
    ++g_run;
    if (ok) return;
    ++g_bad;
    fprintf(stderr, "FAILED: %s %s (last error: %s)\n", what, detail.c_str(), g_error.c_str());
}

// a section in memory: exact allocations
struct Tensor {
    std::unique_ptr<char[]> name;
    std::unique_ptr<float[]> data;
    std::vector<int64_t> shape;
};
struct Section {
    std::vector<Tensor> tensors;
    void add(const std::string& name, std::vector<int64_t> shape, float fill = 0.25f) {
        Tensor t;
        t.name.reset(new char[name.size() + 1]);
        memcpy(t.name.get(), name.c_str(), name.size() + 1);
        int64_t n = 1;
        for (int64_t d : shape) n *= d;
        t.data.reset(new float[(size_t)n]);
        for (int64_t i = 0; i < n; ++i) t.data[(size_t)i] = fill;
        t.shape = shape;
        tensors.push_back(std::move(t));
    }
    void drop(const std::string& name) {
        for (size_t i = 0; i < tensors.size(); ++i)
            if (name == tensors[i].name.get()) {
                tensors.erase(tensors.begin() + (long)i);
                return;
            }
    }
    Tensor* find(const std::string& name) {
        for (Tensor& t : tensors)
            if (name == t.name.get()) return &t;
        return nullptr;
    }
    std::vector<dsd_model_tensor_info> view() const {
        std::vector<dsd_model_tensor_info> out;
        for (const Tensor& t : tensors) {
            dsd_model_tensor_info v;
            memset(&v, 0, sizeof(v));
            v.name = t.name.get();
            v.ndim = (int32_t)t.shape.size();
            v.count = 1;
            for (size_t d = 0; d < t.shape.size(); ++d) {
                v.shape[d] = t.shape[d];
                v.count *= t.shape[d];
            }
            v.data = t.data.get();
            out.push_back(v);
        }
        return out;
    }
};

static dsd_variance_config config_of(bool dur, bool pitch, bool melody, bool glide, bool lang, bool spk, uint32_t variances) {
    dsd_variance_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.hidden_size = 24; c.vocab_size = 7; c.num_lang = lang ? 2 : 0; c.num_spk = spk ? 3 : 0;
    c.predict_dur = dur; c.predict_pitch = pitch; c.use_melody_encoder = melody; c.use_glide_embed = glide;
    c.use_lang_id = lang; c.use_spk_id = spk; c.variances = variances;
    c.melody_hidden_size = melody ? 10 : 0; c.glide_rows = glide ? 3 : 0; c.glide_embed_scale = 11.3f;
    c.smooth_width = pitch ? 5 : 0; c.pitch_repeat_bins = pitch ? 8 : 0;
    c.var_repeat_bins = variances ? 4 : 0;
    c.diffusion_type = 1; c.timesteps = 1000; c.k_step = 1000; c.time_scale_factor = 1000.f;
    return c;
}

static void lin1(Section& s, const std::string& prefix, int64_t h) {
    s.add(prefix + ".weight", {h, 1});
    s.add(prefix + ".bias", {h});
}

static Section section_of(const dsd_variance_config& c) {
    Section s;
    const int64_t H = c.hidden_size, Hm = c.melody_hidden_size;
    s.add("fs2.txt_embed.weight", {c.vocab_size, H});
    if (c.use_lang_id) s.add("fs2.lang_embed.weight", {c.num_lang + 1, H});
    if (c.predict_dur) {
        s.add("fs2.onset_embed.weight", {2, H});
        lin1(s, "fs2.word_dur_embed", H);
        s.add("fs2.midi_embed.weight", {128, H});
    } else {
        lin1(s, "fs2.ph_dur_embed", H);
    }
    if (c.use_spk_id) s.add("spk_embed.weight", {c.num_spk, H});
    if (c.use_melody_encoder) {
        lin1(s, "melody_encoder.note_midi_embed", Hm);
        lin1(s, "melody_encoder.note_dur_embed", Hm);
        if (c.use_glide_embed) s.add("melody_encoder.note_glide_embed.weight", {c.glide_rows, Hm});
    }
    if (c.predict_pitch) {
        s.add("pitch_retake_embed.weight", {2, H});
        lin1(s, c.use_melody_encoder ? "delta_pitch_embed" : "base_pitch_embed", H);
    }
    if (c.variances) {
        lin1(s, "pitch_embed", H);
        for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i)
            if ((c.variances >> i) & 1u) lin1(s, std::string("variance_embeds.") + dsd::kVarianceNames[i], H);
    }
    s.add("cross_lingual_mask", {c.vocab_size}, 0.f);
    s.find("cross_lingual_mask")->data[2] = 1.f;
    return s;
}

static int check(const dsd_variance_config& c, const Section& s, dsd::VarianceTableIndex* ix_out = nullptr) {
    // the index struct on the heap too: a write past it is a heap overflow
    std::unique_ptr<dsd::VarianceTableIndex> ix(new dsd::VarianceTableIndex);
    const std::vector<dsd_model_tensor_info> v = s.view();
    std::unique_ptr<dsd_model_tensor_info[]> exact(new dsd_model_tensor_info[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) exact[i] = v[i];
    g_error.clear();
    const int rc = dsd::variance_tables_check(&c, (int32_t)sizeof(c), exact.get(), (int32_t)v.size(), "harness.tables", ix.get());
    if (ix_out) *ix_out = *ix;
    return rc;
}

static bool refused(int rc, const std::string& word) { return rc == DSD_EINVAL && g_error.find(word) != std::string::npos; }

static void run_combination(const dsd_variance_config& c, const char* tag) {
    Section s = section_of(c);
    dsd::VarianceTableIndex ix;
    expect(check(c, s, &ix) == DSD_OK, "valid section", tag);
    expect(ix.txt >= 0 && ix.mask >= 0 && ix.dur_w >= 0 && ix.dur_b >= 0 && ix.mask_any == 1, "always-present slots", tag);
    expect((ix.lang >= 0) == (c.use_lang_id != 0) && (ix.onset >= 0) == (c.predict_dur != 0) && (ix.midi >= 0) == (c.predict_dur != 0) &&
               (ix.spk >= 0) == (c.use_spk_id != 0) && (ix.note_midi_w >= 0) == (c.use_melody_encoder != 0) &&
               (ix.glide >= 0) == (c.use_glide_embed != 0) && (ix.retake >= 0) == (c.predict_pitch != 0) &&
               (ix.pitch_in_w >= 0) == (c.predict_pitch != 0) && (ix.pitch_w >= 0) == (c.variances != 0),
           "slots follow the flags", tag);
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i)
        expect((ix.var_w[i] >= 0) == (((c.variances >> i) & 1u) != 0) && (ix.var_b[i] >= 0) == (ix.var_w[i] >= 0), "variance slots", tag);

    // every tensor missing in turn; every tensor misshaped four ways
    const std::vector<dsd_model_tensor_info> all = s.view();
    for (const dsd_model_tensor_info& t : all) {
        const std::string name = t.name;
        {
            Section m = section_of(c);
            m.drop(name);
            expect(refused(check(c, m), name) && g_error.find("lacks") != std::string::npos, "missing tensor", name);
        }
        std::vector<std::vector<int64_t>> shapes;
        std::vector<int64_t> base(t.shape, t.shape + t.ndim);
        for (int d = 0; d < t.ndim; ++d) {
            std::vector<int64_t> a = base, b = base;
            a[(size_t)d] += 1;
            b[(size_t)d] -= 1;
            shapes.push_back(a);
            if (b[(size_t)d] >= 1) shapes.push_back(b);
        }
        if (t.ndim == 2 && base[0] != base[1]) shapes.push_back({base[1], base[0]});
        shapes.push_back(t.ndim == 2 ? std::vector<int64_t>{base[0] * base[1]} : std::vector<int64_t>{base[0], 1});
        shapes.push_back({});
        for (const std::vector<int64_t>& shape : shapes) {
            Section m = section_of(c);
            m.drop(name);
            m.add(name, shape, 0.f);
            expect(refused(check(c, m), name) && g_error.find("must be") != std::string::npos, "misshaped tensor", name);
        }
    }
    // tensors the flags exclude, and one nobody knows
    const char* others[] = {"fs2.lang_embed.weight", "fs2.onset_embed.weight", "fs2.word_dur_embed.weight", "fs2.ph_dur_embed.bias",
                            "fs2.midi_embed.weight", "spk_embed.weight", "melody_encoder.note_midi_embed.bias",
                            "melody_encoder.note_glide_embed.weight", "pitch_retake_embed.weight", "delta_pitch_embed.weight",
                            "base_pitch_embed.weight", "pitch_embed.bias", "variance_embeds.energy.weight", "variance_embeds.tension.bias"};
    for (const char* name : others) {
        if (s.find(name)) continue;
        Section m = section_of(c);
        m.add(name, {1});
        expect(refused(check(c, m), name) && g_error.find("excludes") != std::string::npos, "excluded tensor", name);
    }
    {
        Section m = section_of(c);
        m.add("fs2.encoder.layer_norm.weight", {24});
        expect(refused(check(c, m), "fs2.encoder.layer_norm.weight") && g_error.find("do not have") != std::string::npos, "unknown tensor", tag);
    }
    for (float bad : {0.5f, -1.f, 2.f, NAN}) {
        Section m = section_of(c);
        m.find("cross_lingual_mask")->data[(size_t)c.vocab_size - 1] = bad;          // the last float of the allocation
        expect(refused(check(c, m), "cross_lingual_mask[6]"), "mask value", tag);
    }
    {
        Section m = section_of(c);
        m.find("cross_lingual_mask")->data[2] = 0.f;
        dsd::VarianceTableIndex z;
        expect(check(c, m, &z) == DSD_OK && z.mask_any == 0, "an all-zero mask", tag);
    }
    // the optional taps: accepted at [K] with a pitch predictor, refused at another length or without one
    {
        Section m = section_of(c);
        const int64_t K = c.smooth_width > 0 ? c.smooth_width : 5;
        m.add("smooth_taps", {K}, 1.0f / (float)K);
        dsd::VarianceTableIndex z;
        if (c.predict_pitch) {
            expect(check(c, m, &z) == DSD_OK && z.taps >= 0, "stored taps", tag);
            Section n = section_of(c);
            n.add("smooth_taps", {c.smooth_width + 1});
            expect(refused(check(c, n), "smooth_taps") && g_error.find("must be") != std::string::npos, "taps of another length", tag);
            for (float bad : {NAN, INFINITY}) {             // the last float of the allocation
                Section b = section_of(c);
                b.add("smooth_taps", {K}, 1.0f / (float)K);
                b.find("smooth_taps")->data[(size_t)K - 1] = bad;
                expect(refused(check(c, b), "smooth_taps[4] is not finite"), "a tap that is not finite", tag);
            }
            Section o = section_of(c);
            o.add("smooth_taps", {K}, 0.25f);
            expect(refused(check(c, o), "smooth_taps sum to 1.25"), "taps that do not sum to 1", tag);
            dsd_variance_config one = c;
            one.smooth_width = 1;
            Section q = section_of(one);
            q.add("smooth_taps", {1}, NAN);
            expect(check(one, q) == DSD_OK, "K = 1 takes the reference's NaN tap", tag);
        } else {
            expect(refused(check(c, m), "smooth_taps") && g_error.find("excludes") != std::string::npos, "taps without a pitch predictor", tag);
        }
        expect(ix.taps == -1, "no taps stored", tag);
    }
    // the config's own rules
    if (c.predict_pitch)
        for (int k : {0, -1, 256, 1 << 20}) {
            dsd_variance_config b = c;
            b.smooth_width = k;
            expect(refused(check(b, s), "smooth_width"), "K outside 1 .. 255", tag);
        }
    for (int k : {1, 255}) {
        dsd_variance_config b = c;
        b.smooth_width = k;
        expect(check(b, s) == DSD_OK, "K at its limits", tag);
    }
    {
        dsd_variance_config b = c;
        b.use_spk_id = 2;
        expect(refused(check(b, s), "use_spk_id = 2"), "flag value", tag);
        b = c;
        b.variances |= 16u;
        expect(refused(check(b, s), "variances"), "variance bits", tag);
        b = c;
        b.struct_size -= 4;
        expect(refused(check(b, s), "struct_size"), "struct_size", tag);
        b = c;
        b.hidden_size = 0;
        expect(refused(check(b, s), "hidden_size"), "hidden_size", tag);
        b = c;
        b.diffusion_type = 2;
        expect(refused(check(b, s), "diffusion_type"), "diffusion_type", tag);
        b = c;
        b.var_no_clamp[3] = -1;
        expect(refused(check(b, s), "var_no_clamp[3]"), "var_no_clamp", tag);
    }
    expect(dsd::variance_tables_check(&c, (int32_t)sizeof(c) - 4, nullptr, 0, "harness.tables", &ix) == DSD_EINVAL, "config size", tag);
    expect(dsd::variance_tables_check(nullptr, (int32_t)sizeof(c), nullptr, 0, "harness.tables", &ix) == DSD_EINVAL, "NULL config", tag);
    expect(dsd::variance_tables_check(&c, (int32_t)sizeof(c), nullptr, 3, "harness.tables", &ix) == DSD_EINVAL, "NULL tensors", tag);
}

static void run_inner() {
    const dsd_variance_config c = config_of(true, true, true, true, true, true, 1u | 8u);
    dsd_token_encoder_config fs2, mel;
    memset(&fs2, 0, sizeof(fs2));
    fs2.struct_size = sizeof(fs2); fs2.hidden_size = 24; fs2.dur_layers = 2;
    mel = fs2;
    mel.hidden_size = 10; mel.out_dims = 24; mel.dur_layers = 0;
    dsd_config pit, var;
    memset(&pit, 0, sizeof(pit));
    pit.struct_size = sizeof(pit); pit.hidden_size = 24; pit.in_dims = 8; pit.n_feats = 1;
    var = pit;
    var.in_dims = 4; var.n_feats = 2;
    expect(dsd::variance_inner_check(&c, &fs2, &mel, &pit, &var) == DSD_OK, "valid inner configs");
    struct { const char* words[2]; int which; int field; int value; } cases[] = {
        {{"fs2.hidden_size = 32", "tables.hidden_size = 24"}, 0, 0, 32}, {{"fs2.out_dims = 24", "out_dims"}, 0, 1, 24},
        {{"fs2.dur_layers = 0", "tables.predict_dur = 1"}, 0, 2, 0}, {{"melody.hidden_size = 24", "tables.melody_hidden_size = 10"}, 1, 0, 24},
        {{"melody.out_dims = 10", "tables.hidden_size = 24"}, 1, 1, 10}, {{"melody.dur_layers = 2", "dur_layers"}, 1, 2, 2},
        {{"pitch.hidden_size = 64", "tables.hidden_size = 24"}, 2, 0, 64}, {{"pitch.in_dims = 4", "tables.pitch_repeat_bins = 8"}, 2, 1, 4},
        {{"pitch.n_feats = 2", "n_feats"}, 2, 2, 2}, {{"variances.hidden_size = 8", "tables.hidden_size = 24"}, 3, 0, 8},
        {{"variances.in_dims = 8", "tables.var_repeat_bins = 4"}, 3, 1, 8}, {{"variances.n_feats = 1", "tables.variances"}, 3, 2, 1}};
    for (const auto& k : cases) {
        dsd_token_encoder_config f = fs2, m = mel;
        dsd_config p = pit, v = var;
        if (k.which < 2) {
            dsd_token_encoder_config& t = k.which ? m : f;
            (k.field == 0 ? t.hidden_size : k.field == 1 ? t.out_dims : t.dur_layers) = k.value;
        } else {
            dsd_config& t = k.which == 2 ? p : v;
            (k.field == 0 ? t.hidden_size : k.field == 1 ? t.in_dims : t.n_feats) = k.value;
        }
        g_error.clear();
        const int rc = dsd::variance_inner_check(&c, &f, &m, &p, &v);
        expect(refused(rc, k.words[0]) && g_error.find(k.words[1]) != std::string::npos, "inner mismatch", k.words[0]);
    }
    expect(dsd::variance_inner_check(&c, &fs2, nullptr, &pit, &var) == DSD_EINVAL, "missing melody config");
    expect(dsd::variance_inner_check(&c, &fs2, &mel, nullptr, &var) == DSD_EINVAL, "missing pitch config");
    expect(dsd::variance_inner_check(&c, &fs2, &mel, &pit, nullptr) == DSD_EINVAL, "missing variances config");
    const dsd_variance_config plain = config_of(false, false, false, false, false, false, 0);
    fs2.dur_layers = 0;
    expect(dsd::variance_inner_check(&plain, &fs2, nullptr, nullptr, nullptr) == DSD_OK, "an encoder-only model");
}

static void run_taps() {
    for (int K = 1; K <= 255; ++K) {
        std::unique_ptr<float[]> w(new float[(size_t)K]);
        dsd::variance_smooth_taps(K, w.get());
        if (K == 1) {
            expect(isnan(w[0]), "K = 1 is 0 / 0");
            continue;
        }
        double sum = 0;
        bool ok = true;
        for (int k = 0; k < K; ++k) {
            ok = ok && isfinite(w[k]);
            sum += w[k];
        }
        expect(ok && fabs(sum - 1.0) < 1e-5, "taps", std::to_string(K));
    }
    // the bits, for tests/test_cvariance_host.py to hold against its restatement of the formula
    for (int K : {1, 2, 3, 4, 5, 21, 64, 255}) {
        std::unique_ptr<float[]> w(new float[(size_t)K]);
        dsd::variance_smooth_taps(K, w.get());
        printf("taps %d", K);
        for (int k = 0; k < K; ++k) {
            uint32_t bits;
            memcpy(&bits, &w[k], 4);
            printf(" %08x", bits);
        }
        printf("\n");
    }
}

int main() {
    run_combination(config_of(true, true, true, true, true, true, 0), "word form, melody, glide, language, speaker");
    run_combination(config_of(true, true, false, false, false, false, 0), "word form, base pitch");
    run_combination(config_of(false, true, true, false, false, false, 0), "phoneme form, melody without glides");
    run_combination(config_of(false, false, false, false, false, false, 1u), "one variance");
    run_combination(config_of(false, false, false, false, false, true, 1u | 4u | 8u), "three variances, speaker");
    run_combination(config_of(true, true, true, true, true, true, 15u), "everything");
    run_combination(config_of(false, false, false, false, false, false, 0), "the encoder alone");
    run_inner();
    run_taps();
    printf("variance_harness: %d checks, %d failed\n", g_run, g_bad);
    return g_bad ? 1 : 0;
}
