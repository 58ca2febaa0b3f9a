// Stand-alone memory check of the host-only half of the acoustic twin (diffsinger_amd/csrc/acoustic_tables.hip), under the
// host compiler's address and undefined-behaviour sanitizers.  Builds tables sections in memory - every tensor its own heap
// allocation of exactly count floats, every name its own exact allocation - for a set of flag combinations, and runs
//   1. the valid section of each combination: DSD_OK, every slot the config requires filled, none it excludes;
//   2. each refusal on each combination where it applies: a tensor missing, one the config excludes, an unknown one, every
//      tensor with a dimension one short, one long or of another rank, a mask value that is not 0 / 1, spec_max not above
//      spec_min at the last bin, a flag that is not 0 / 1, the shift and speed ranges, a wrong struct_size - a negative code
//      and a message naming the tensor or field;
//   3. the inner-config check: valid, and one mismatch per field it compares;
//   4. dsd_acoustic_plan over steps 1 .. 60 x a grid of depths for both diffusion types: the invariants of the plan (the
//      start follows t_max / t_start, the DDPM coefficients are the schedule's and square to 1 together, the ancestral
//      sampler's noise count), and every DSD_EINVAL of the call.  The plan reads two schedule tables at t_max - 1: a read
//      past them is what the sanitizer reports.
// Host only - never loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/acoustic_harness.cpp -x c++ diffsinger_amd/csrc/acoustic_tables.hip diffsinger_amd/csrc/program_api.hip
//       -o /tmp/acoustic_harness
//   /tmp/acoustic_harness        # prints one line of counts; exit status 0 = clean
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

#include "../../diffsinger_amd/csrc/acoustic_tables.h"

// the layout tests/test_cacoustic_host.py pins from the Python side, from the C side
static_assert(sizeof(dsd_acoustic_config) == 96, "dsd_acoustic_config is 24 words");
static_assert(offsetof(dsd_acoustic_config, out_dims) == 12 && offsetof(dsd_acoustic_config, embed_flags) == 32 &&
                  offsetof(dsd_acoustic_config, shift_min) == 44 && offsetof(dsd_acoustic_config, mel_base_e) == 60 &&
                  offsetof(dsd_acoustic_config, schedule_type) == 76 && offsetof(dsd_acoustic_config, max_beta) == 80 &&
                  offsetof(dsd_acoustic_config, t_start) == 88 && offsetof(dsd_acoustic_config, time_scale_factor) == 92,
              "dsd_acoustic_config layout");
static_assert(sizeof(dsd_acoustic_plan_t) == 36 && offsetof(dsd_acoustic_plan_t, t_start) == 16 && offsetof(dsd_acoustic_plan_t, steps) == 32,
              "dsd_acoustic_plan_t layout");
static_assert(sizeof(dsd_acoustic_condition_args) == 136 && offsetof(dsd_acoustic_condition_args, curves) == 40 &&
                  offsetof(dsd_acoustic_condition_args, languages) == 104 && offsetof(dsd_acoustic_condition_args, f0_coarse) == 128,
              "dsd_acoustic_condition_args layout");

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

static dsd_acoustic_config config_of(bool discrete, bool lang, bool spk, uint32_t flags, bool shallow, int type) {
    dsd_acoustic_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.hidden_size = 24; c.vocab_size = 7; c.out_dims = 5; c.num_lang = lang ? 2 : 0; c.num_spk = spk ? 3 : 0;
    c.use_lang_id = lang; c.use_spk_id = spk; c.embed_flags = flags; c.f0_discrete = discrete; c.use_shallow_diffusion = shallow;
    if (flags & DSD_EMBED_KEY_SHIFT) { c.shift_min = -5.f; c.shift_max = 5.f; }
    if (flags & DSD_EMBED_SPEED) { c.speed_min = 0.5f; c.speed_max = 2.f; }
    c.diffusion_type = type;
    if (type == DSD_DIFFUSE_DDPM) {
        c.timesteps = 1000; c.k_step = shallow ? 400 : 1000; c.schedule_type = DSD_SCHEDULE_LINEAR; c.max_beta = 0.01;
    } else {
        c.t_start = shallow ? 0.4f : 0.f; c.time_scale_factor = 1000.f;
    }
    return c;
}

static Section section_of(const dsd_acoustic_config& c, bool frozen) {
    Section s;
    s.add("cross_lingual_mask", {c.vocab_size}, 0.f);
    s.find("cross_lingual_mask")->data[2] = 1.f;
    s.add("spec_min", {c.out_dims}, -12.f);
    s.add("spec_max", {c.out_dims}, 0.5f);
    if (c.f0_discrete) s.add("fs2.pitch_embed.weight", {DSD_AC_PITCH_BINS, c.hidden_size});
    if (frozen && c.use_spk_id) s.add("frozen_spk_embed", {c.hidden_size});
    if (frozen && (c.embed_flags & DSD_EMBED_KEY_SHIFT)) s.add("frozen_key_shift", {1}, 2.f);
    return s;
}

static int check(const dsd_acoustic_config& c, const Section& s, dsd::AcousticTableIndex* ix_out = nullptr) {
    // the index struct on the heap too: a write past it is a heap overflow
    std::unique_ptr<dsd::AcousticTableIndex> ix(new dsd::AcousticTableIndex);
    const std::vector<dsd_model_tensor_info> v = s.view();
    std::unique_ptr<dsd_model_tensor_info[]> exact(new dsd_model_tensor_info[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) exact[i] = v[i];
    g_error.clear();
    const int rc = dsd::acoustic_tables_check(&c, (int32_t)sizeof(c), exact.get(), (int32_t)v.size(), "harness.tables", ix.get());
    if (ix_out) *ix_out = *ix;
    return rc;
}

static bool refused(int rc, const std::string& word) { return rc == DSD_EINVAL && g_error.find(word) != std::string::npos; }

static void run_combination(const dsd_acoustic_config& c, bool frozen, const char* tag) {
    Section s = section_of(c, frozen);
    dsd::AcousticTableIndex ix;
    expect(check(c, s, &ix) == DSD_OK, "valid section", tag);
    expect(ix.mask >= 0 && ix.spec_min >= 0 && ix.spec_max >= 0 && ix.mask_any == 1, "always-present slots", tag);
    expect((ix.pitch_embed >= 0) == (c.f0_discrete != 0) && (ix.frozen_spk >= 0) == (frozen && c.use_spk_id) &&
               (ix.frozen_key_shift >= 0) == (frozen && (c.embed_flags & DSD_EMBED_KEY_SHIFT) != 0),
           "slots follow the config", tag);
    const std::vector<dsd_model_tensor_info> all = s.view();
    for (const dsd_model_tensor_info& t : all) {
        const std::string name = t.name;
        const bool optional = name.rfind("frozen_", 0) == 0;
        {
            Section m = section_of(c, frozen);
            m.drop(name);
            if (optional) expect(check(c, m) == DSD_OK, "an optional tensor left out", name);
            else expect(refused(check(c, m), name) && g_error.find("lacks") != std::string::npos, "missing tensor", name);
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
        if (t.ndim == 2) shapes.push_back({base[1], base[0]});
        shapes.push_back(t.ndim == 2 ? std::vector<int64_t>{base[0] * base[1]} : std::vector<int64_t>{base[0], 1});
        shapes.push_back({});
        for (const std::vector<int64_t>& shape : shapes) {
            Section m = section_of(c, frozen);
            m.drop(name);
            m.add(name, shape, 0.f);
            expect(refused(check(c, m), name) && g_error.find("must be") != std::string::npos, "misshaped tensor", name);
        }
    }
    for (const char* name : {"fs2.pitch_embed.weight", "frozen_spk_embed", "frozen_key_shift"}) {
        const bool allowed = std::string(name) == "fs2.pitch_embed.weight" ? c.f0_discrete != 0
                             : std::string(name) == "frozen_spk_embed"     ? c.use_spk_id != 0
                                                                           : (c.embed_flags & DSD_EMBED_KEY_SHIFT) != 0;
        if (allowed) continue;
        Section m = section_of(c, frozen);
        m.add(name, {1});
        expect(refused(check(c, m), name) && g_error.find("excludes") != std::string::npos, "excluded tensor", name);
    }
    {
        Section m = section_of(c, frozen);
        m.add("fs2.txt_embed.weight", {7, 24});
        expect(refused(check(c, m), "fs2.txt_embed.weight") && g_error.find("do not have") != std::string::npos, "unknown tensor", tag);
    }
    for (float bad : {0.5f, -1.f, 2.f, NAN}) {
        Section m = section_of(c, frozen);
        m.find("cross_lingual_mask")->data[(size_t)c.vocab_size - 1] = bad;          // the last float of the allocation
        expect(refused(check(c, m), "cross_lingual_mask[6]"), "mask value", tag);
    }
    {
        Section m = section_of(c, frozen);
        m.find("cross_lingual_mask")->data[2] = 0.f;
        dsd::AcousticTableIndex z;
        expect(check(c, m, &z) == DSD_OK && z.mask_any == 0, "an all-zero mask", tag);
    }
    for (float bad : {-12.f, -13.f, NAN, INFINITY}) {
        Section m = section_of(c, frozen);
        m.find("spec_max")->data[(size_t)c.out_dims - 1] = bad;                       // the last float of the allocation
        expect(refused(check(c, m), "spec_max[4]"), "spec_max not above spec_min", tag);
    }
    // the config's own rules
    {
        dsd_acoustic_config b = c;
        b.mel_base_e = 2;
        expect(refused(check(b, s), "mel_base_e = 2"), "flag value", tag);
        b = c;
        b.f0_discrete = -1;
        expect(refused(check(b, s), "f0_discrete = -1"), "flag value", tag);
        b = c;
        b.embed_flags |= 64u;
        expect(refused(check(b, s), "embed_flags"), "embed bits", tag);
        b = c;
        b.struct_size -= 4;
        expect(refused(check(b, s), "struct_size"), "struct_size", tag);
        b = c;
        b.out_dims = 0;
        expect(refused(check(b, s), "out_dims"), "out_dims", tag);
        b = c;
        b.diffusion_type = 2;
        expect(refused(check(b, s), "diffusion_type"), "diffusion_type", tag);
        if (c.embed_flags & DSD_EMBED_KEY_SHIFT) {
            b = c;
            b.shift_min = 1.f;
            expect(refused(check(b, s), "shift_min"), "shift_min above 0", tag);
            b = c;
            b.shift_max = -1.f;
            expect(refused(check(b, s), "shift_max"), "shift_max below 0", tag);
        }
        if (c.embed_flags & DSD_EMBED_SPEED) {
            b = c;
            b.speed_min = 0.f;
            expect(refused(check(b, s), "speed_min"), "speed_min of 0", tag);
            b = c;
            b.speed_max = 0.25f;
            expect(refused(check(b, s), "speed_max"), "speed_max below speed_min", tag);
        }
        if (c.diffusion_type == DSD_DIFFUSE_DDPM) {
            b = c;
            b.k_step = 1001;
            expect(refused(check(b, s), "k_step"), "k_step above timesteps", tag);
            b = c;
            b.max_beta = 0.0;
            expect(refused(check(b, s), "max_beta"), "max_beta", tag);
        } else {
            b = c;
            b.t_start = 1.5f;
            expect(refused(check(b, s), "t_start"), "t_start", tag);
        }
    }
    expect(dsd::acoustic_tables_check(&c, (int32_t)sizeof(c) - 4, nullptr, 0, "harness.tables", &ix) == DSD_EINVAL, "config size", tag);
    expect(dsd::acoustic_tables_check(nullptr, (int32_t)sizeof(c), nullptr, 0, "harness.tables", &ix) == DSD_EINVAL, "NULL config", tag);
    expect(dsd::acoustic_tables_check(&c, (int32_t)sizeof(c), nullptr, 3, "harness.tables", &ix) == DSD_EINVAL, "NULL tensors", tag);
}

static void run_inner() {
    const dsd_acoustic_config c = config_of(true, true, true, 1u | 16u | 32u, true, DSD_DIFFUSE_DDPM);
    dsd_encoder_config fs2;
    memset(&fs2, 0, sizeof(fs2));
    fs2.struct_size = sizeof(fs2); fs2.hidden_size = 24; fs2.vocab_size = 7; fs2.embed_flags = 1u | 16u | 32u; fs2.num_spk = 3; fs2.num_lang = 2;
    dsd_config den, aux;
    memset(&den, 0, sizeof(den));
    den.struct_size = sizeof(den); den.hidden_size = 24; den.in_dims = 5; den.n_feats = 1;
    aux = den;
    aux.backbone = DSD_AUX_CONVNEXT;
    expect(dsd::acoustic_inner_check(&c, &fs2, &den, &aux) == DSD_OK, "valid inner configs");
    struct { const char* words[2]; int which; int field; int value; } cases[] = {
        {{"fs2.hidden_size = 32", "tables.hidden_size = 24"}, 0, 0, 32}, {{"fs2.vocab_size = 8", "tables.vocab_size = 7"}, 0, 1, 8},
        {{"fs2.embed_flags = 1", "tables.embed_flags = 49"}, 0, 2, 1}, {{"fs2.num_spk = 0", "tables.num_spk = 3"}, 0, 3, 0},
        {{"fs2.num_lang = 1", "tables.num_lang = 2"}, 0, 4, 1},
        {{"denoiser.in_dims = 80", "tables.out_dims = 5"}, 1, 0, 80}, {{"denoiser.n_feats = 2", "n_feats"}, 1, 1, 2},
        {{"denoiser.hidden_size = 8", "tables.hidden_size = 24"}, 1, 2, 8},
        {{"aux.in_dims = 4", "tables.out_dims = 5"}, 2, 0, 4}, {{"aux.n_feats = 3", "n_feats"}, 2, 1, 3},
        {{"aux.hidden_size = 64", "tables.hidden_size = 24"}, 2, 2, 64}};
    for (const auto& k : cases) {
        dsd_encoder_config f = fs2;
        dsd_config d = den, a = aux;
        if (k.which == 0) {
            if (k.field == 2) f.embed_flags = (uint32_t)k.value;
            else (k.field == 0 ? f.hidden_size : k.field == 1 ? f.vocab_size : k.field == 3 ? f.num_spk : f.num_lang) = k.value;
        } else {
            dsd_config& t = k.which == 1 ? d : a;
            (k.field == 0 ? t.in_dims : k.field == 1 ? t.n_feats : t.hidden_size) = k.value;
        }
        g_error.clear();
        const int rc = dsd::acoustic_inner_check(&c, &f, &d, &a);
        expect(refused(rc, k.words[0]) && g_error.find(k.words[1]) != std::string::npos, "inner mismatch", k.words[0]);
    }
    expect(dsd::acoustic_inner_check(&c, &fs2, &den, nullptr) == DSD_EINVAL, "missing aux config");
    expect(dsd::acoustic_inner_check(&c, nullptr, &den, &aux) == DSD_EINVAL, "missing encoder config");
    expect(dsd::acoustic_inner_check(&c, &fs2, nullptr, &aux) == DSD_EINVAL, "missing denoiser config");
    dsd_acoustic_config plain = config_of(false, false, false, 0, false, DSD_DIFFUSE_REFLOW);
    fs2.embed_flags = 0; fs2.num_spk = 0; fs2.num_lang = 0;
    expect(dsd::acoustic_inner_check(&plain, &fs2, &den, nullptr) == DSD_OK, "a model without shallow diffusion");
}

static void run_plan() {
    const float depths[] = {-1.f, 0.f, 0.001f, 0.004f, 0.06f, 0.3f, 0.4f, 0.9f, 1.f, 1.5f};
    for (int k_step : {400, 1000, 0})
        for (const char* kind : {"linear", "cosine"}) {
            dsd_acoustic_config c = config_of(false, false, false, 0, true, DSD_DIFFUSE_DDPM);
            c.k_step = k_step;
            c.schedule_type = kind[0] == 'l' ? DSD_SCHEDULE_LINEAR : DSD_SCHEDULE_COSINE;
            std::unique_ptr<float[]> tables(new float[(size_t)DSD_DDPM_TABLES * 1000]);
            expect(dsd_ddpm_tables_fill(c.schedule_type, 1000, c.max_beta, tables.get()) == DSD_OK, "the schedule", kind);
            for (int steps = 1; steps <= 60; ++steps)
                for (float depth : depths) {
                    std::unique_ptr<dsd_acoustic_plan_t> p(new dsd_acoustic_plan_t);
                    const std::string tag = std::to_string(k_step) + " " + std::to_string(steps) + " " + std::to_string(depth);
                    if (dsd_acoustic_plan(&c, depth, steps, p.get()) != DSD_OK) {
                        expect(false, "DDPM plan", tag);
                        continue;
                    }
                    bool ok = p->mode == DSD_DIFFUSE_DDPM && p->steps == steps && p->t_max >= 0 && p->t_max <= k_step && p->speedup >= 1 &&
                              p->n_step_noise == (p->speedup == 1 ? p->t_max : 0);
                    if (depth < 0) {
                        ok = ok && p->t_max == k_step && 1000 % p->speedup == 0 && p->start == DSD_AC_START_NOISE;
                    } else {
                        ok = ok && p->t_max % p->speedup == 0;
                        if (p->t_max >= 1000) ok = ok && p->start == DSD_AC_START_NOISE && p->src_scale == 0.f && p->noise_scale == 1.f;
                        else if (p->t_max == 0) ok = ok && p->start == DSD_AC_START_SOURCE && p->src_scale == 1.f && p->noise_scale == 0.f;
                        else
                            ok = ok && p->start == DSD_AC_START_MIX && p->src_scale == tables[3 * 1000 + (size_t)p->t_max - 1] &&
                                 p->noise_scale == tables[4 * 1000 + (size_t)p->t_max - 1] &&
                                 fabs((double)p->src_scale * p->src_scale + (double)p->noise_scale * p->noise_scale - 1.0) < 1e-6;
                    }
                    expect(ok, "DDPM plan invariants", tag);
                }
        }
    for (float t0 : {0.f, 0.4f, 1.f}) {
        dsd_acoustic_config c = config_of(false, false, false, 0, true, DSD_DIFFUSE_REFLOW);
        c.t_start = t0;
        for (int steps = -1; steps <= 60; ++steps)
            for (float depth : depths) {
                std::unique_ptr<dsd_acoustic_plan_t> p(new dsd_acoustic_plan_t);
                const std::string tag = std::to_string(t0) + " " + std::to_string(steps) + " " + std::to_string(depth);
                if (dsd_acoustic_plan(&c, depth, steps, p.get()) != DSD_OK) {
                    expect(false, "reflow plan", tag);
                    continue;
                }
                const float want = depth < 0 ? 0.f : fmaxf(1.0f - depth, t0);
                bool ok = p->mode == DSD_DIFFUSE_REFLOW && p->steps == steps && p->t_max == 0 && p->speedup == 0 && p->n_step_noise == 0 &&
                          p->t_start == want;
                if (want <= 0.f) ok = ok && p->start == DSD_AC_START_NOISE && p->src_scale == 0.f && p->noise_scale == 1.f;
                else if (want >= 1.f) ok = ok && p->start == DSD_AC_START_SOURCE && p->src_scale == 1.f && p->noise_scale == 0.f;
                else ok = ok && p->start == DSD_AC_START_MIX && p->src_scale == want && p->noise_scale == (float)(1.0 - (double)want);
                expect(ok, "reflow plan invariants", tag);
            }
    }
    // every refusal
    dsd_acoustic_config c = config_of(false, false, false, 0, true, DSD_DIFFUSE_DDPM);
    dsd_acoustic_plan_t p;
    expect(dsd_acoustic_plan(nullptr, 0.3f, 4, &p) == DSD_EINVAL && g_error.find("NULL") != std::string::npos, "NULL config");
    expect(dsd_acoustic_plan(&c, 0.3f, 4, nullptr) == DSD_EINVAL && g_error.find("NULL") != std::string::npos, "NULL plan");
    expect(refused(dsd_acoustic_plan(&c, NAN, 4, &p), "NaN"), "a NaN depth");
    expect(refused(dsd_acoustic_plan(&c, 0.3f, 0, &p), "steps = 0"), "steps = 0 on DDPM");
    expect(refused(dsd_acoustic_plan(&c, -1.f, -3, &p), "steps = -3"), "negative steps on DDPM");
    dsd_acoustic_config b = c;
    b.struct_size = 92;
    expect(refused(dsd_acoustic_plan(&b, 0.3f, 4, &p), "struct_size"), "struct_size");
    b = c;
    b.diffusion_type = 7;
    expect(refused(dsd_acoustic_plan(&b, 0.3f, 4, &p), "diffusion_type = 7"), "diffusion_type");
    b = c;
    b.timesteps = 0;
    expect(refused(dsd_acoustic_plan(&b, 0.3f, 4, &p), "timesteps = 0"), "timesteps");
    b = c;
    b.schedule_type = 5;
    expect(dsd_acoustic_plan(&b, 0.3f, 4, &p) == DSD_EINVAL, "schedule_type (dsd_ddpm_tables_fill's refusal)");
    dsd_acoustic_config r = config_of(false, false, false, 0, true, DSD_DIFFUSE_REFLOW);
    expect(refused(dsd_acoustic_plan(&r, NAN, 4, &p), "NaN"), "a NaN depth on reflow");
    expect(dsd_acoustic_plan(&r, 0.5f, 0, &p) == DSD_OK && p.start == DSD_AC_START_MIX, "reflow takes steps = 0 (the empty loop)");
}

int main() {
    const uint32_t all = 63u;
    run_combination(config_of(true, true, true, all, true, DSD_DIFFUSE_DDPM), true, "everything, frozen tensors");
    run_combination(config_of(true, true, true, all, true, DSD_DIFFUSE_REFLOW), false, "everything, reflow");
    run_combination(config_of(false, false, false, 0, false, DSD_DIFFUSE_DDPM), false, "the plain model");
    run_combination(config_of(false, false, true, DSD_EMBED_SPEED, false, DSD_DIFFUSE_REFLOW), true, "speaker and speed, frozen speaker");
    run_combination(config_of(true, false, false, DSD_EMBED_KEY_SHIFT | DSD_EMBED_ENERGY, true, DSD_DIFFUSE_REFLOW), true,
                    "discrete f0, frozen key shift");
    run_inner();
    run_plan();
    printf("acoustic_harness: %d checks, %d failed\n", g_run, g_bad);
    return g_bad ? 1 : 0;
}
