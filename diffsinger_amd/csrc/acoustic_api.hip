// libdsdenoise, the acoustic model's staged twin on one model file: dsd_acoustic_open / _close / _info / _handle and the
// stage calls dsd_acoustic_condition, _start and _sample.  Host code on top of the library's own public calls - the model
// file reader, dsd_model_create, dsd_length_regulate, dsd_encode, dsd_cond_assemble, dsd_aux_decode, dsd_prepare_cond,
// dsd_program_build, dsd_sample - plus the launches of acoustic_kernels.hip, in the order diffsinger_amd/deploy.py and
// diffusion.py's forward_onnx give them, so a stage's output is bit-identical to the Python twin's on the same operands.
// The host-only checks of a tables section and dsd_acoustic_plan are acoustic_tables.hip.
#include "api_host.h"
#include "acoustic_tables.h"

struct dsd_acoustic {
    dsd_acoustic_config cfg;
    int device = 0;
    AcousticTableIndex ix;
    bool lang_on = false;               // use_lang_id and a set entry in the cross-lingual mask
    dsd_handle *fs2 = nullptr, *aux = nullptr, *denoiser = nullptr;
    DevBuf<float> consts;               // k [M], mid [M], then the tables section's tensors
    const float *k = nullptr, *mid = nullptr, *mask = nullptr, *pitch_embed = nullptr, *frozen_spk = nullptr, *frozen_key_shift = nullptr;
    float coarse_a = 0.f, coarse_b = 0.f;
    std::vector<float> ddpm_tables;     // HOST [12][timesteps] (DDPM)
    // the sampler programs built so far, per plan: one, or the ancestral sampler's chunks in order
    std::map<std::vector<int32_t>, std::vector<dsd_program*>> programs;
    // one workspace per stage, grown on demand: a call at sizes already met allocates nothing, and a graph captured over a
    // stage stays valid until that stage is called with larger sizes
    DevBuf<char> ws_cond, ws_sample;
    // dsd_acoustic_set_lengths: the lengths the stage calls check their (B, T) against; the inner handles hold their own copies
    bool ragged = false;
    std::vector<int32_t> lengths;
    SpkMixIds spk_ids;                  // dsd_acoustic_spk_mix's ids on the device
    void drop_programs() {
        for (auto& kv : programs)
            for (dsd_program* p : kv.second) dsd_program_free(p);
        programs.clear();
    }
    ~dsd_acoustic() {
        drop_programs();
        for (dsd_handle* h : {fs2, aux, denoiser})
            if (h) dsd_destroy(h);
    }
};

namespace {

constexpr int kMaxItems = 65535;        // the batch rides in gridDim.y / .z
constexpr int kAncestralChunk = 50;     // diffusion.py's _ANCESTRAL_CHUNK: steps per dsd_sample call
constexpr size_t kMaxPrograms = 32;
const char* const kCurveNames[4] = {"energy", "breathiness", "voicing", "tension"};
const dsd_program kNoop = {1, 0, 0, 0, nullptr};        // schedule.Program(1, 0, []): the result is x itself

// carves a stage's workspace: sizes first (p == nullptr), then the pointers
struct Carver {
    char* p;
    size_t used = 0;
    explicit Carver(char* base) : p(base) {}
    template <typename T>
    T* take(size_t n) {
        used = (used + 255) & ~(size_t)255;
        T* out = p ? reinterpret_cast<T*>(p + used) : nullptr;
        used += n * sizeof(T);
        return out;
    }
};

std::string last(dsd_handle* h) { return std::string(dsd_last_error(h)); }

#define LIB_OK(who, call, what)                                                                  \
    do {                                                                                         \
        const int rc_ = (call);                                                                  \
        if (rc_ != DSD_OK) return fail(nullptr, rc_, "%s: %s: %s", who, what, last(nullptr).c_str()); \
    } while (0)
#define HANDLE_OK(who, h, call, what)                                                            \
    do {                                                                                         \
        const int rc_ = (call);                                                                  \
        if (rc_ != DSD_OK) return fail(nullptr, rc_, "%s: %s: %s", who, what, last(h).c_str());  \
    } while (0)
#define LAUNCH_OK(who, call, what)                                                               \
    do {                                                                                         \
        const hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: %s launch failed: %s", who, what, hipGetErrorString(e_)); \
    } while (0)

int check_sizes(const char* who, int B, int L, int T) {
    if (B < 1 || B > kMaxItems) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, %d]", who, B, kMaxItems);
    if (L != -1 && (L < 1 || L > kRegulateMaxTokens)) return fail(nullptr, DSD_EINVAL, "%s: L = %d outside [1, %d]", who, L, kRegulateMaxTokens);
    if (T < 1) return fail(nullptr, DSD_EINVAL, "%s: T = %d must be positive", who, T);
    if ((int64_t)B * T > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: B * T = %lld exceeds 2^31 - 1", who, (long long)B * T);
    return DSD_OK;
}

// dsd_set_lengths' rules for the stage calls, checked by the object itself: dsd_acoustic_start and a condition stage without an
// aux decoder reach no inner handle that would
int check_lengths(const dsd_acoustic* a, const char* who, int B, int T) {
    if (!a->ragged) return DSD_OK;
    if ((int)a->lengths.size() != B)
        return fail(nullptr, DSD_ESTATE, "%s: dsd_acoustic_set_lengths gave %d lengths but this call runs a batch of %d", who,
                    (int)a->lengths.size(), B);
    for (int b = 0; b < B; ++b)
        if (a->lengths[(size_t)b] > T) return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d exceeds T = %d", who, b, a->lengths[(size_t)b], T);
    return DSD_OK;
}

int section_of(const dsd_model_file* f, const std::string& name, const char* who, dsd_model_section_info* info) {
    const int i = dsd_model_find(f, name.c_str());
    if (i < 0) return fail(nullptr, DSD_ENOTFOUND, "%s: the file has no section \"%s\"", who, name.c_str());
    if (int rc = dsd_model_section(f, i, info)) return rc;
    return i + 1;       // > 0: the index plus one
}

int open_impl(const dsd_model_file* f, const char* prefix, int32_t device, dsd_acoustic* a) {
    const char* who = "dsd_acoustic_open";
    const std::string pre(prefix);
    dsd_model_section_info info;
    int rc = section_of(f, pre + ".tables", who, &info);
    if (rc < 0) return rc;
    const int tables_i = rc - 1;
    if (info.kind != DSD_ACOUSTIC_TABLES)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not DSD_ACOUSTIC_TABLES (%d)", who, info.name, info.kind, DSD_ACOUSTIC_TABLES);
    if (info.config_size != (int32_t)sizeof(dsd_acoustic_config))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": config of %d bytes", who, info.name, info.config_size);
    LIB_OK(who, dsd_model_config(f, tables_i, &a->cfg, info.config_size), "the tables' config");
    std::vector<dsd_model_tensor_info> tensors((size_t)info.n_tensors);
    for (int32_t j = 0; j < info.n_tensors; ++j) LIB_OK(who, dsd_model_tensor(f, tables_i, j, &tensors[(size_t)j]), "a table");
    if (int r = acoustic_tables_check(&a->cfg, info.config_size, tensors.data(), info.n_tensors, info.name, &a->ix)) return r;
    const dsd_acoustic_config& c = a->cfg;
    a->lang_on = c.use_lang_id && a->ix.mask_any;

    // the inner sections: kinds and configs, still on the host
    dsd_encoder_config ecfg;
    dsd_config dcfg, acfg;
    int fs2_i, den_i, aux_i = -1;
    {
        dsd_model_section_info si;
        if ((rc = section_of(f, pre + ".fs2", who, &si)) < 0) return rc;
        fs2_i = rc - 1;
        if (si.kind != DSD_ENC_FS2_ACOUSTIC)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not an acoustic encoder (%d)", who, si.name, si.kind, DSD_ENC_FS2_ACOUSTIC);
        LIB_OK(who, dsd_model_config(f, fs2_i, &ecfg, sizeof(ecfg)), si.name);
        if (c.use_shallow_diffusion) {
            if ((rc = section_of(f, pre + ".aux", who, &si)) < 0) return rc;
            aux_i = rc - 1;
            if (si.kind != DSD_AUX_CONVNEXT)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not an aux decoder (%d)", who, si.name, si.kind, DSD_AUX_CONVNEXT);
            LIB_OK(who, dsd_model_config(f, aux_i, &acfg, sizeof(acfg)), si.name);
        }
        if ((rc = section_of(f, pre + ".denoiser", who, &si)) < 0) return rc;
        den_i = rc - 1;
        if (si.kind != DSD_BACKBONE_WAVENET && si.kind != DSD_BACKBONE_LYNXNET)
            return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not a denoiser (%d or %d)", who, si.name, si.kind,
                        DSD_BACKBONE_WAVENET, DSD_BACKBONE_LYNXNET);
        LIB_OK(who, dsd_model_config(f, den_i, &dcfg, sizeof(dcfg)), si.name);
    }
    if (int r = acoustic_inner_check(&c, &ecfg, &dcfg, c.use_shallow_diffusion ? &acfg : nullptr)) return r;
    if (c.diffusion_type == DSD_DIFFUSE_DDPM) {
        a->ddpm_tables.resize((size_t)DSD_DDPM_TABLES * (size_t)c.timesteps);
        LIB_OK(who, dsd_ddpm_tables_fill(c.schedule_type, c.timesteps, c.max_beta, a->ddpm_tables.data()), "the schedule");
    }
    {   // f0_to_coarse's constants (fastspeech2.py:14-28), in double as numpy forms them, rounded to fp32 where torch meets them
        const double mel_min = 1127.0 * log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * log(1.0 + 1100.0 / 700.0);
        const double ca = (256.0 - 2.0) / (mel_max - mel_min), cb = mel_min * ca - 1.0;
        a->coarse_a = (float)ca;
        a->coarse_b = (float)cb;
    }

    // the device: inner handles, then the constants in one block
    if (int r = select_device(who, device)) return r;
    a->device = device;
    LIB_OK(who, dsd_model_create(f, fs2_i, device, &a->fs2), "the encoder");
    if (aux_i >= 0) LIB_OK(who, dsd_model_create(f, aux_i, device, &a->aux), "the aux decoder");
    LIB_OK(who, dsd_model_create(f, den_i, device, &a->denoiser), "the denoiser");
    const size_t M = (size_t)c.out_dims;
    std::vector<float> host;
    auto align = [&] { host.resize((host.size() + 63) / 64 * 64, 0.f); };
    const float *lo = tensors[(size_t)a->ix.spec_min].data, *hi = tensors[(size_t)a->ix.spec_max].data;
    for (size_t m = 0; m < M; ++m) host.push_back((hi[m] - lo[m]) * 0.5f);      // k = (spec_max - spec_min) / 2 in fp32
    align();
    const size_t mid_off = host.size();
    for (size_t m = 0; m < M; ++m) host.push_back((hi[m] + lo[m]) * 0.5f);      // mid = (spec_max + spec_min) / 2
    align();
    size_t off[4] = {0, 0, 0, 0};
    const int which[4] = {a->ix.mask, a->ix.pitch_embed, a->ix.frozen_spk, a->ix.frozen_key_shift};
    for (int i = 0; i < 4; ++i) {
        if (which[i] < 0) continue;
        off[i] = host.size();
        const dsd_model_tensor_info& t = tensors[(size_t)which[i]];
        host.insert(host.end(), t.data, t.data + t.count);
        align();
    }
    if (int r = a->consts.reserve(nullptr, host.size(), who)) return r;
    HIP_OK(nullptr, hipMemcpy(a->consts.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    a->k = a->consts.p;
    a->mid = a->consts.p + mid_off;
    a->mask = a->consts.p + off[0];
    a->pitch_embed = which[1] >= 0 ? a->consts.p + off[1] : nullptr;
    a->frozen_spk = which[2] >= 0 ? a->consts.p + off[2] : nullptr;
    a->frozen_key_shift = which[3] >= 0 ? a->consts.p + off[3] : nullptr;
    return DSD_OK;
}

// the plan's programs, built on first use: one, or the ancestral sampler's chunks from t_max down
int programs_of(dsd_acoustic* a, const dsd_acoustic_plan_t& p, const char* who, const std::vector<dsd_program*>** out) {
    const dsd_acoustic_config& c = a->cfg;
    int32_t t_bits;
    memcpy(&t_bits, &p.t_start, sizeof(t_bits));
    const bool reflow = p.mode == DSD_DIFFUSE_REFLOW;
    const std::vector<int32_t> key = {p.mode, reflow ? 0 : p.t_max, reflow ? 0 : p.speedup, reflow ? p.steps : 0, reflow ? t_bits : 0};
    auto it = a->programs.find(key);
    if (it == a->programs.end()) {
        if (a->programs.size() >= kMaxPrograms) a->drop_programs();
        std::vector<dsd_program*> built;
        dsd_sampler_spec s;
        memset(&s, 0, sizeof(s));
        s.struct_size = sizeof(s);
        int rc = DSD_OK;
        if (p.mode == DSD_DIFFUSE_REFLOW) {
            s.sampler = DSD_SAMPLER_RF_EULER_ONNX;
            s.steps = p.steps;
            s.t_start = (double)p.t_start;
            s.time_scale_factor = (double)c.time_scale_factor;
            dsd_program* prog = nullptr;
            if ((rc = dsd_program_build(&s, &prog)) == DSD_OK) built.push_back(prog);
        } else {
            s.timesteps = c.timesteps;
            s.tables = a->ddpm_tables.data();
            s.speedup = p.speedup;
            if (p.speedup > 1) {
                s.sampler = DSD_SAMPLER_DDIM;
                s.t_max = p.t_max;
                dsd_program* prog = nullptr;
                if ((rc = dsd_program_build(&s, &prog)) == DSD_OK) built.push_back(prog);
            } else {
                s.sampler = DSD_SAMPLER_DDPM;
                for (int hi = p.t_max; hi > 0 && rc == DSD_OK; hi = s.t_lo) {
                    s.t_max = hi;
                    s.t_lo = std::max(hi - kAncestralChunk, 0);
                    dsd_program* prog = nullptr;
                    if ((rc = dsd_program_build(&s, &prog)) == DSD_OK) built.push_back(prog);
                }
            }
        }
        if (rc != DSD_OK) {
            const std::string why = last(nullptr);
            for (dsd_program* q : built) dsd_program_free(q);
            return fail(nullptr, rc, "%s: the sampler program: %s", who, why.c_str());
        }
        it = a->programs.emplace(key, std::move(built)).first;
    }
    *out = &it->second;
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_acoustic_open(const dsd_model_file* f, const char* prefix, int32_t device, dsd_acoustic** out) {
    const char* who = "dsd_acoustic_open";
    if (out) *out = nullptr;
    if (!f || !prefix || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    if (strlen(prefix) > DSD_MODEL_MAX_NAME - 10) return fail(nullptr, DSD_EINVAL, "%s: the prefix is longer than %d bytes", who, DSD_MODEL_MAX_NAME - 10);
    dsd_acoustic* a = nullptr;
    int rc;
    try {
        a = new dsd_acoustic();
        memset(&a->cfg, 0, sizeof(a->cfg));
        rc = open_impl(f, prefix, device, a);
    } catch (const std::exception&) {
        rc = fail(nullptr, DSD_ENOMEM, "%s: out of host memory", who);
    }
    if (rc != DSD_OK) {
        const std::string why = last(nullptr);      // the destructor's calls must not replace the message
        delete a;
        return fail(nullptr, rc, "%s", why.c_str());
    }
    *out = a;
    return DSD_OK;
}

void dsd_acoustic_close(dsd_acoustic* a) { delete a; }

int dsd_acoustic_info(const dsd_acoustic* a, dsd_acoustic_config* out) {
    if (!a || !out) return fail(nullptr, DSD_EINVAL, "dsd_acoustic_info: NULL argument");
    *out = a->cfg;
    return DSD_OK;
}

int dsd_acoustic_handle(const dsd_acoustic* a, int32_t which, dsd_handle** out) {
    const char* who = "dsd_acoustic_handle";
    if (out) *out = nullptr;
    if (!a || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    if (which != DSD_AC_FS2 && which != DSD_AC_AUX && which != DSD_AC_DENOISER)
        return fail(nullptr, DSD_EINVAL, "%s: which = %d is none of DSD_AC_FS2, DSD_AC_AUX, DSD_AC_DENOISER", who, which);
    dsd_handle* h = which == DSD_AC_FS2 ? a->fs2 : (which == DSD_AC_AUX ? a->aux : a->denoiser);
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: the model has no aux decoder (use_shallow_diffusion = 0)", who);
    *out = h;
    return DSD_OK;
}

int dsd_acoustic_condition(dsd_acoustic* a, const dsd_acoustic_condition_args* g, void* stream) {
    const char* who = "dsd_acoustic_condition";
    if (!a) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!g) return fail(nullptr, DSD_EINVAL, "%s: NULL args", who);
    if (g->struct_size != (int32_t)sizeof(*g)) return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(*g));
    const dsd_acoustic_config& c = a->cfg;
    if (!g->tokens || !g->durations || !g->f0 || !g->condition) return fail(nullptr, DSD_EINVAL, "%s: NULL tokens, durations, f0 or condition", who);
    if (int rc = check_sizes(who, g->B, g->L, g->T)) return rc;
    if (int rc = check_lengths(a, who, g->B, g->T)) return rc;
    for (int i = 0; i < 4; ++i) {
        const bool set = (c.embed_flags >> i) & 1u;
        if (set && !g->curves[i]) return fail(nullptr, DSD_EINVAL, "%s: NULL curves[%d] (%s), which the model embeds", who, i, kCurveNames[i]);
        if (!set && g->curves[i]) return fail(nullptr, DSD_EINVAL, "%s: curves[%d] (%s) given, but the model has no such embedding", who, i, kCurveNames[i]);
    }
    const bool key_shift = c.embed_flags & DSD_EMBED_KEY_SHIFT, speed = c.embed_flags & DSD_EMBED_SPEED;
    if (key_shift && !a->frozen_key_shift && !g->gender)
        return fail(nullptr, DSD_EINVAL, "%s: NULL gender on a model with a key-shift embedding and no frozen_key_shift", who);
    if (!key_shift && g->gender) return fail(nullptr, DSD_EINVAL, "%s: gender given, but the model has no key-shift embedding", who);
    if (!speed && g->velocity) return fail(nullptr, DSD_EINVAL, "%s: velocity given, but the model has no speed embedding", who);
    if (g->spk_embed) {
        if (!c.use_spk_id) return fail(nullptr, DSD_EINVAL, "%s: spk_embed given, but the model has no speaker embedding (use_spk_id = 0)", who);
        if (g->spk_rows != 1 && g->spk_rows != g->T) return fail(nullptr, DSD_EINVAL, "%s: spk_rows = %d is neither 1 nor T = %d", who, g->spk_rows, g->T);
    } else if (c.use_spk_id && !a->frozen_spk) {
        return fail(nullptr, DSD_EINVAL, "%s: NULL spk_embed on a model with a speaker embedding and no frozen_spk_embed", who);
    }
    if (a->lang_on && !g->languages) return fail(nullptr, DSD_EINVAL, "%s: languages is required: the model's cross-lingual mask has a set entry", who);
    if (c.use_shallow_diffusion && !g->aux_mel) return fail(nullptr, DSD_EINVAL, "%s: NULL aux_mel on a model with shallow diffusion", who);
    if (!c.use_shallow_diffusion && g->aux_mel) return fail(nullptr, DSD_EINVAL, "%s: aux_mel given, but the model has no aux decoder (use_shallow_diffusion = 0)", who);
    if (!c.f0_discrete && g->f0_coarse) return fail(nullptr, DSD_EINVAL, "%s: f0_coarse given, but the model embeds f0 continuously (f0_discrete = 0)", who);
    const int B = g->B, L = g->L, T = g->T, H = c.hidden_size;
    const size_t nl = (size_t)B * L, nt = (size_t)B * T;
    const bool discrete = c.f0_discrete != 0;
    HIP_OK(nullptr, hipSetDevice(a->device));       // before the workspace is sized: it lives on the object's device
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? a->ws_cond.p : nullptr);
        int64_t* dur_m = cv.take<int64_t>(nl);
        int64_t* lang = cv.take<int64_t>(c.use_lang_id ? nl : 0);
        int64_t* mel2ph = cv.take<int64_t>(nt);
        float* f0_m = cv.take<float>(nt);
        float* f0_enc = cv.take<float>(discrete ? nt : 0);
        float* ks = cv.take<float>(key_shift ? nt : 0);
        float* sp = cv.take<float>(speed ? nt : 0);
        int64_t* iota = cv.take<int64_t>(discrete ? nt : 0);
        int64_t* coarse = cv.take<int64_t>(discrete ? nt : 0);
        float* enc_out = cv.take<float>(discrete ? nt * H : 0);
        if (!pass) {
            if (int rc = a->ws_cond.reserve(nullptr, cv.used, who)) return rc;
            continue;
        }
        hipStream_t st = (hipStream_t)stream;
        AcTokensP tp;
        memset(&tp, 0, sizeof(tp));
        tp.tokens = (const long long*)g->tokens; tp.durations = (const long long*)g->durations;
        tp.languages = a->lang_on ? (const long long*)g->languages : nullptr;
        tp.mask = a->mask; tp.L = L; tp.vocab = c.vocab_size;
        tp.dur_m = (long long*)dur_m; tp.lang = c.use_lang_id ? (long long*)lang : nullptr;
        LAUNCH_OK(who, launch_ac_tokens(tp, B, st), "the token kernel");
        LIB_OK(who, dsd_length_regulate(a->device, dur_m, B, L, T, mel2ph, stream), "mel2ph");
        AcFramesP fp;
        memset(&fp, 0, sizeof(fp));
        fp.mel2ph = (const long long*)mel2ph; fp.f0 = g->f0; fp.gender = g->gender; fp.velocity = g->velocity;
        fp.frozen_key_shift = a->frozen_key_shift; fp.T = T;
        fp.shift_max = c.shift_max; fp.shift_min_abs = fabsf(c.shift_min); fp.speed_min = c.speed_min; fp.speed_max = c.speed_max;
        fp.inv_700 = 1.0f / 700.0f; fp.coarse_a = a->coarse_a; fp.coarse_b = a->coarse_b;
        fp.f0_m = f0_m; fp.f0_enc = discrete ? f0_enc : nullptr;
        fp.key_shift = key_shift ? ks : nullptr; fp.speed = speed ? sp : nullptr;
        fp.iota = discrete ? (long long*)iota : nullptr; fp.coarse = discrete ? (long long*)coarse : nullptr;
        fp.coarse_out = (long long*)g->f0_coarse;
        LAUNCH_OK(who, launch_ac_frames(fp, B, st), "the frame kernel");
        dsd_encode_extras ex;
        memset(&ex, 0, sizeof(ex));
        if (c.use_lang_id) ex.languages = lang;
        if (c.use_spk_id) {
            if (a->frozen_spk) {
                ex.spk_mix_embed = a->frozen_spk;       // [1, 1, H], broadcast over the items and the frames
            } else {
                ex.spk_mix_embed = g->spk_embed;
                ex.spk_mix_bstride = (int64_t)g->spk_rows * H;
                ex.spk_mix_tstride = g->spk_rows > 1 ? H : 0;
            }
        }
        if (key_shift) ex.key_shift = ks;
        if (speed) ex.speed = sp;
        ex.energy = g->curves[0]; ex.breathiness = g->curves[1]; ex.voicing = g->curves[2]; ex.tension = g->curves[3];
        HANDLE_OK(who, a->fs2, dsd_encode(a->fs2, g->tokens, mel2ph, discrete ? f0_enc : f0_m, B, L, T, &ex, discrete ? enc_out : g->condition, stream),
                  "the encoder");
        if (discrete) {     // condition + pitch_embed.weight[f0_to_coarse(f0)], the gathers in deploy.py's order
            dsd_assemble_args as;
            memset(&as, 0, sizeof(as));
            as.struct_size = sizeof(as);
            as.device = a->device;
            as.B = B; as.T = T; as.H = H;
            as.n_gather = 2;
            as.gather[0].table = enc_out; as.gather[0].batch_stride = (int64_t)T * H; as.gather[0].rows = T; as.gather[0].idx = iota;
            as.gather[0].idx_offset = 0; as.gather[0].scale = 1.0f;
            as.gather[1].table = a->pitch_embed; as.gather[1].batch_stride = 0; as.gather[1].rows = DSD_AC_PITCH_BINS; as.gather[1].idx = coarse;
            as.gather[1].idx_offset = 0; as.gather[1].scale = 1.0f;
            LIB_OK(who, dsd_cond_assemble(&as, g->condition, stream), "the discrete f0 embedding");
        }
        if (c.use_shallow_diffusion)
            HANDLE_OK(who, a->aux, dsd_aux_decode(a->aux, g->condition, B, T, (int64_t)T * H, 1, H, g->aux_mel, a->k, a->mid, stream), "the aux decoder");
    }
    return DSD_OK;
}

int dsd_acoustic_start(dsd_acoustic* a, const dsd_acoustic_plan_t* plan, const float* source, const float* noise, int32_t B, int32_t T,
                       float* x, void* stream) {
    const char* who = "dsd_acoustic_start";
    if (!a) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!plan || !x) return fail(nullptr, DSD_EINVAL, "%s: NULL plan or x", who);
    if (int rc = check_sizes(who, B, -1, T)) return rc;
    if (int rc = check_lengths(a, who, B, T)) return rc;
    const int M = a->cfg.out_dims;
    if ((int64_t)B * T * M > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: B * M * T = %lld exceeds 2^31 - 1", who, (long long)B * T * M);
    if (plan->start != DSD_AC_START_NOISE && plan->start != DSD_AC_START_MIX && plan->start != DSD_AC_START_SOURCE)
        return fail(nullptr, DSD_EINVAL, "%s: plan->start = %d is none of DSD_AC_START_NOISE, _MIX, _SOURCE", who, plan->start);
    if (plan->start == DSD_AC_START_NOISE && !noise) return fail(nullptr, DSD_EINVAL, "%s: NULL noise for a start from noise", who);
    if (plan->start != DSD_AC_START_NOISE && !source) return fail(nullptr, DSD_EINVAL, "%s: NULL source for a start from the shallow source", who);
    if (x == source || x == noise) return fail(nullptr, DSD_EINVAL, "%s: x must not alias source or noise", who);
    HIP_OK(nullptr, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    if (plan->start == DSD_AC_START_NOISE) {
        HIP_OK(nullptr, hipMemcpyAsync(x, noise, sizeof(float) * (size_t)B * T * M, hipMemcpyDeviceToDevice, st));
        return DSD_OK;
    }
    const float* mix = plan->start == DSD_AC_START_MIX ? noise : nullptr;
    LAUNCH_OK(who, launch_ac_source(source, mix, a->k, a->mid, plan->src_scale, plan->noise_scale, B, M, T, x, st), "the source kernel");
    return DSD_OK;
}

int dsd_acoustic_sample(dsd_acoustic* a, const dsd_acoustic_plan_t* plan, const float* condition, const float* x, const float* step_noise,
                        int32_t B, int32_t T, uint32_t flags, float* mel, void* stream) {
    const char* who = "dsd_acoustic_sample";
    if (!a) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!plan || !condition || !x || !mel) return fail(nullptr, DSD_EINVAL, "%s: NULL plan, condition, x or mel", who);
    if (int rc = check_sizes(who, B, -1, T)) return rc;
    if (int rc = check_lengths(a, who, B, T)) return rc;
    const dsd_acoustic_config& c = a->cfg;
    const int M = c.out_dims, H = c.hidden_size;
    if ((int64_t)B * T * M > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: B * M * T = %lld exceeds 2^31 - 1", who, (long long)B * T * M);
    if (flags & ~(uint32_t)(DSD_SAMPLE_GRAPH | DSD_SAMPLE_GRAPH_LAZY))
        return fail(nullptr, DSD_EINVAL, "%s: flags = 0x%x: only DSD_SAMPLE_GRAPH and DSD_SAMPLE_GRAPH_LAZY are the caller's", who, flags);
    if (plan->mode != c.diffusion_type)
        return fail(nullptr, DSD_EINVAL, "%s: plan->mode = %d, but the model's diffusion_type is %d", who, plan->mode, c.diffusion_type);
    bool noop;
    if (plan->mode == DSD_DIFFUSE_DDPM) {
        if (plan->t_max < 0 || plan->t_max > c.timesteps || plan->speedup < 1)
            return fail(nullptr, DSD_EINVAL, "%s: plan->t_max = %d outside [0, %d] or plan->speedup = %d below 1", who, plan->t_max, c.timesteps, plan->speedup);
        if (plan->n_step_noise != (plan->speedup == 1 ? plan->t_max : 0))
            return fail(nullptr, DSD_EINVAL, "%s: plan->n_step_noise = %d does not belong to t_max = %d, speedup = %d", who, plan->n_step_noise,
                        plan->t_max, plan->speedup);
        noop = plan->t_max == 0;
    } else {
        if (!(plan->t_start >= 0.f) || plan->n_step_noise != 0)
            return fail(nullptr, DSD_EINVAL, "%s: plan->t_start = %g must not be negative, plan->n_step_noise = %d must be 0", who,
                        (double)plan->t_start, plan->n_step_noise);
        noop = plan->t_start >= 1.f || plan->steps < 1;
    }
    if (plan->n_step_noise > 0 && !step_noise) return fail(nullptr, DSD_EINVAL, "%s: NULL step_noise, but the plan reads %d tensors", who, plan->n_step_noise);
    const std::vector<dsd_program*>* progs = nullptr;
    if (!noop)
        if (int rc = programs_of(a, *plan, who, &progs)) return rc;
    const size_t n = (size_t)B * T * M;
    const size_t chunks = noop ? 1 : progs->size();
    HIP_OK(nullptr, hipSetDevice(a->device));
    float* pong[2] = {nullptr, nullptr};
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? a->ws_sample.p : nullptr);
        pong[0] = cv.take<float>(chunks > 1 ? n : 0);
        pong[1] = cv.take<float>(chunks > 2 ? n : 0);
        if (!pass)
            if (int rc = a->ws_sample.reserve(nullptr, cv.used, who)) return rc;
    }
    dsd_handle* h = a->denoiser;
    HANDLE_OK(who, h, dsd_prepare_cond(h, condition, B, T, (int64_t)T * H, 1, H, stream), "dsd_prepare_cond");
    const float* cur = x;
    int used = 0;
    for (size_t i = 0; i < chunks; ++i) {
        const dsd_program* prog = noop ? &kNoop : (*progs)[i];
        const bool final_chunk = i + 1 == chunks;
        float* dst = final_chunk ? mel : pong[i & 1];
        const float* eps = prog->n_noise > 0 ? step_noise + (size_t)used * n : nullptr;      // consumed in order
        HANDLE_OK(who, h, dsd_sample(h, prog, cur, eps, dst, final_chunk ? a->k : nullptr, final_chunk ? a->mid : nullptr,
                                     (final_chunk ? DSD_SAMPLE_TRANSPOSE : 0u) | flags, stream), "dsd_sample");
        used += prog->n_noise;
        cur = dst;
    }
    if (!c.mel_base_e) LAUNCH_OK(who, launch_ac_mel_base(mel, (long)n, 2.30259f, (hipStream_t)stream), "the mel base kernel");
    return DSD_OK;
}

int dsd_acoustic_set_lengths(dsd_acoustic* a, const int32_t* lengths, int32_t B, void* stream) {
    const char* who = "dsd_acoustic_set_lengths";
    if (!a) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (lengths) {      // everything dsd_set_lengths would refuse, first: the two handles are then set both, or neither
        if (B < 1 || B > kMaxItems) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, %d]", who, B, kMaxItems);
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 0) return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d is negative", who, b, lengths[b]);
    }
    if (a->aux) HANDLE_OK(who, a->aux, dsd_set_lengths(a->aux, lengths, B, stream), "the aux decoder");
    HANDLE_OK(who, a->denoiser, dsd_set_lengths(a->denoiser, lengths, B, stream), "the denoiser");
    a->ragged = lengths != nullptr;
    if (lengths) a->lengths.assign(lengths, lengths + B);
    else a->lengths.clear();
    return DSD_OK;
}

int dsd_acoustic_spk_mix(dsd_acoustic* a, const dsd_spk_mix_args* args, void* stream) {
    const char* who = "dsd_acoustic_spk_mix";
    if (!a) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    const dsd_acoustic_config& c = a->cfg;
    const char* why_not = nullptr;
    if (!c.use_spk_id) why_not = "the model has no speaker embedding (use_spk_id = 0)";
    else if (a->frozen_spk) why_not = "the model's speaker is frozen (frozen_spk_embed): there is nothing to mix";
    else if (a->fs2->e_spk == SIZE_MAX) why_not = "the encoder holds no spk_embed.weight";
    const float* table = why_not ? nullptr : a->fs2->blob.p + a->fs2->e_spk;      // the table the encoder handle holds
    return spk_mix_run(who, args, table, why_not ? why_not : "", c.num_spk, c.hidden_size, a->device, a->spk_ids, stream);
}

}  // extern "C"
